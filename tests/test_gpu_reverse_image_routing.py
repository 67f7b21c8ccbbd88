"""Per-image routing of the two fused reverse kernels: sc_sdf_backward_fused (csrc/sdf_bwdw.hip) and the fused forms of the RGB /
compositing reverse (csrc/rgb_bwd.hip).  Both map a tile / a ray to its image inside a persistent two-role workgroup to form the
per-image bias gradients g_cbias [B, 5, 64] / g_dbias [B, 3, 64] -- the latent gradients of the implicit networks -- through several
branches: one accumulator while a 4-tile / 4-ray iteration stays in one image, a per-tile "mixed" branch when it straddles images,
float atomics beyond 256 images (SDF only), workgroups without work that must still write a zero partial image.  The cases of
tests/reverse_routing_cases.py sit on those branches (proved on the host by tests/test_reverse_partition_host.py).

A routing error moves a few tiles' worth of bias gradient into a neighbour's row: inside a tolerance when images are large.  So,
besides (a) the float64 budget of tests/test_gpu_float64_budget.py (its oracles, its K, its rule (b)),
  (b) leak, exact: with the cotangents of all images but one zeroed, every gradient row of every other image is == 0;
  (c) batch independence, exact: d L / d points of image b out of the batch is torch.equal to a one-image run on image b.
Every test prints its three-arm table and the worst ratio to the fp32 oracle per class (recorded in tests/reverse_routing_cases.py and
docs/LAB_NOTEBOOK.md)."""
import functools
import os
import sys
from contextlib import contextmanager, nullcontext

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reverse_routing_cases as C  # noqa: E402
import test_gpu_float64_budget as F  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HIP_ERROR_INVALID_VALUE = 1


def _worst(title, rows, K):
    """Per class, the worst default / twins error in units of the fp32 oracle's (what the case tables record; only errors above the
    2^-22 floor count, below it a ratio says nothing) and the largest share of the bound K err(oracle) + 2^-22 that rule (b) allows."""
    ratio, share = {}, {}
    for c, d, t, o in rows.values():
        share[c] = max(share.get(c, 0.0), max(d, t) / (K[c] * o + F.FLOOR))
        if max(d, t) > F.FLOOR:
            ratio[c] = max(ratio.get(c, 0.0), max(d, t) / max(o, 1e-30))
    print("worst of default / twins, %s: %s" % (title, "  ".join("%s %.2f x oracle (%.2f of the bound)" % (c, ratio.get(c, 0.0), share[c])
                                                                 for c in sorted(share))))


# ---------------------------------------------------------------------------------------------------------------------------------
# SDF
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sdf_case(B, N):
    """Weights, latents, points and cotangents (sdf, d sdf/dx, feature) of a case: drawn as test_sdf_backward_fused_float64_budget does."""
    from oracle import reference_ops as R
    cfg = R.Cfg()
    g = torch.Generator().manual_seed(B * 7 + N)
    W = {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in R.init_sdf_weights(cfg, 1).items()}
    z = torch.randn(B, 64, generator=g)
    pts = torch.rand(B * N, 3, generator=g) * 2 - 1
    c = (torch.randn(B * N, generator=g), torch.randn(B * N, 3, generator=g), torch.randn(B * N, 64, generator=g) * 0.1)
    return cfg, W, z, pts, c


def _image(B, N, b, hot=False):
    """The one-image case of image b; hot: the whole batch with every other image's cotangents zeroed."""
    cfg, W, z, pts, c = _sdf_case(B, N)
    s = slice(b * N, (b + 1) * N)
    if not hot:
        return W, z[b:b + 1], pts[s], tuple(x[s] for x in c)
    ch = tuple(torch.zeros_like(x) for x in c)
    for x, y in zip(ch, c):
        x[s] = y[s]
    return W, z, pts, ch


def _sdf_direct(W, z, pts, c, N):
    """SdfFunction forward + backward, the gradients taken at the kernel's own inputs: (g_pack, g_cbias [B, 5, 64], g_points) on the CPU."""
    from shapeclipper_amd import packing
    from shapeclipper_amd.functional import SdfFunction
    Wd = {k: v.to(DEV).requires_grad_(True) for k, v in W.items()}
    zd, pd = z.to(DEV).requires_grad_(True), pts.to(DEV).requires_grad_(True)
    pack, cb = packing.pack_sdf(Wd, zd)
    sdf, grad, feat = SdfFunction.apply(pd, pack, cb, N, True, True, True, True)
    L = (sdf * c[0].to(DEV)).sum() + (grad * c[1].to(DEV)).sum() + (packing.tbl_to_rows(feat, pts.shape[0]) * c[2].to(DEV)).sum()
    gs = torch.autograd.grad(L, [pack, cb, pd])
    torch.cuda.synchronize()
    return [x.cpu() for x in gs]


SDF_BUDGET = [(B, N, True) for B, N in C.SDF_CASES] + [C.SDF_FEAT_ABSENT + (False,)]


@pytest.mark.parametrize("B,N,feat", SDF_BUDGET)
def test_sdf_fused_reverse_float64_budget(B, N, feat):
    """(a) every weight, latent and point gradient against the float64 double backward, rule (b) of _check with K_SDF_BWD (both HIP arms
    run the same reverse kernel: no rule (a), as in test_sdf_backward_fused_float64_budget).  feat False: g_feat is absent."""
    cfg, W, z, pts, c = _sdf_case(B, N)
    c = c if feat else (c[0], c[1], None)
    r64, r32 = F._sdf_bwd_oracle(cfg, W, z, pts, c, B, torch.float64), F._sdf_bwd_oracle(cfg, W, z, pts, c, B, torch.float32)
    d = F._sdf_bwd_hip(W, z, pts, c, N)
    with F._twins():
        t = F._sdf_bwd_hip(W, z, pts, c, N)
    if not feat:
        assert float(d["lin5.weight"][1:].abs().max()) == 0.0 and float(d["lin5.bias"][1:].abs().max()) == 0.0
    rows = {k: ("w_sdf" if k.startswith("lin") else k, F._err(d[k], r64[k]), F._err(t[k], r64[k]), F._err(r32[k], r64[k])) for k in r64}
    title = "SDF fused reverse B=%d N=%d feat=%s" % (B, N, feat)
    _worst(title, rows, F.K_SDF_BWD)
    F._check(title, rows, F.K_SDF_BWD, rule_a=False)


@pytest.mark.parametrize("B,N", C.SDF_LEAK_CASES)
def test_sdf_fused_reverse_leaks_nothing_into_other_images(B, N):
    """(b) one hot image h in {0, B // 2, B - 1}: the g_cbias rows and the g_points rows of every other image are exactly zero, in the
    dense and in the atomic form; image h's rows against float64 within (a)'s budget.  The oracle runs on image h alone: under these
    cotangents every other image's terms are products with an exact zero, in any precision, so d L / d lin_l.bias IS g_cbias[h, l]."""
    cfg = _sdf_case(B, N)[0]
    for h in C.hot_images(B):
        W, z, pts, ch = _image(B, N, h, hot=True)
        _, g_cb, g_p = _sdf_direct(W, z, pts, ch, N)
        with F._twins():
            _, t_cb, t_p = _sdf_direct(W, z, pts, ch, N)
        other = torch.ones(B, dtype=torch.bool)
        other[h] = False
        for arm, cb, gp in (("default", g_cb, g_p), ("twins", t_cb, t_p)):
            assert cb.shape == (B, 5, 64) and gp.shape == (B * N, 3)
            n_cb, n_p = int((cb[other] != 0).sum()), int((gp.view(B, N, 3)[other] != 0).sum())
            assert n_cb == 0 and n_p == 0, "%s arm, hot image %d: %d g_cbias and %d g_points elements of other images are not zero " \
                "(images %s)" % (arm, h, n_cb, n_p, sorted(set(torch.nonzero(cb.abs().amax((1, 2)) * other)[:, 0].tolist()))[:8])
            assert float(cb[h].abs().max()) > 0 and float(gp.view(B, N, 3)[h].abs().max()) > 0
        W1, z1, p1, c1 = _image(B, N, h)
        r64, r32 = F._sdf_bwd_oracle(cfg, W1, z1, p1, c1, 1, torch.float64), F._sdf_bwd_oracle(cfg, W1, z1, p1, c1, 1, torch.float32)
        s = slice(h * N, (h + 1) * N)
        rows = {"g_cbias[%d, %d]" % (h, l): ("w_sdf", F._err(g_cb[h, l], r64["lin%d.bias" % l]), F._err(t_cb[h, l], r64["lin%d.bias" % l]),
                                             F._err(r32["lin%d.bias" % l], r64["lin%d.bias" % l])) for l in range(5)}
        rows["g_points[image %d]" % h] = ("points", F._err(g_p[s], r64["points"]), F._err(t_p[s], r64["points"]), F._err(r32["points"], r64["points"]))
        title = "SDF fused reverse B=%d N=%d, hot image %d" % (B, N, h)
        _worst(title, rows, F.K_SDF_BWD)
        F._check(title, rows, F.K_SDF_BWD, rule_a=False)


@pytest.mark.parametrize("B,N", C.SDF_BATCH_CASES)
def test_sdf_fused_reverse_point_gradients_do_not_depend_on_the_batch(B, N):
    """(c) g_points of image b out of the batched run is bit-equal to a B = 1 run on image b's points, latent and cotangents: a tile's
    chain reads its own 16 points, the shared weight image and its image's biases, whichever workgroup, wave and iteration it falls to."""
    cfg, W, z, pts, c = _sdf_case(B, N)
    for twins in (False, True):
        with (F._twins() if twins else nullcontext()):
            batched = F._sdf_bwd_hip(W, z, pts, c, N)["points"]
            for b in C.hot_images(B):
                alone = F._sdf_bwd_hip(*_image(B, N, b), N)["points"]
                got = batched[b * N:(b + 1) * N]
                assert alone.shape == (N, 3) and float(alone.abs().min()) > 0
                assert torch.equal(got, alone), "image %d (twins %s): %d of %d elements differ, largest difference %g" % (
                    b, twins, int((got != alone).sum()), alone.numel(), float((got - alone).abs().max()))


def test_sdf_fused_reverse_refuses_before_any_launch():
    """n_per_image % 16 != 0, n_images <= 0 and a null g_cbias with 257 images return hipErrorInvalidValue before anything is
    launched (no argument is dereferenced: every pointer is the same 16-float tensor)."""
    from shapeclipper_amd import _lib
    lib = _lib.load()
    x = torch.zeros(16, device=DEV)
    p = _lib.ptr(x)

    def call(n_points, n_per_image, n_images, g_cbias):
        return lib.sc_sdf_backward_fused(p, p, n_points, n_per_image, n_images, 1, p, p, p, p, p, p, p, p, g_cbias, _lib.stream())
    assert call(48, 24, 2, p) == HIP_ERROR_INVALID_VALUE
    assert call(48, 0, 3, p) == HIP_ERROR_INVALID_VALUE
    assert call(48, 16, 0, p) == HIP_ERROR_INVALID_VALUE
    assert call(48, 16, -3, p) == HIP_ERROR_INVALID_VALUE
    assert call(257 * 16, 16, 257, None) == HIP_ERROR_INVALID_VALUE
    assert call(0, 16, 3, p) == 0                                  # an empty point set: nothing to do, no error
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0


def test_sdf_backward_fused_on_an_empty_point_set_returns_zeros():
    from shapeclipper_amd import ops, packing
    pts = torch.zeros(0, 3, device=DEV)
    w = torch.zeros(packing.SDF_PACK_FLOATS, device=DEV)
    for n_images in (3, 257):
        g_p, g_w, g_c = ops.sdf_backward_fused(pts, w, 16, n_images, True, None, None, None, None, None)
        assert g_p.shape == (0, 3) and g_w.shape == (packing.SDF_PACK_FLOATS,) and g_c.shape == (n_images, 5, 64)
        assert all(t.is_cuda and t.dtype == torch.float32 for t in (g_p, g_w, g_c))
        assert float(g_w.abs().max()) == 0.0 and float(g_c.abs().max()) == 0.0
    assert ops.sdf_backward_fused(pts, w, 16, 3, True, None, None, None, None, None, want_points_grad=False)[0] is None


# ---------------------------------------------------------------------------------------------------------------------------------
# RGB
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rgb_refs(n_images, rpi, S):
    return F._rgb_refs(n_images, rpi, S)


@contextmanager
def _reverse_entries():
    """Names of the RGB reverse entry points ops.rgb_composite_backward resolves (ops._entry) inside the block."""
    from shapeclipper_amd import ops
    names, real = [], ops._entry

    def spy(lib, name, S):
        if "backward" in name:
            names.append((name, S))
        return real(lib, name, S)
    ops._entry = spy
    try:
        yield names
    finally:
        ops._entry = real


def _fused_ran(names, n_images, S, form):
    from shapeclipper_amd import ops
    assert ops.rgb_forward_parks(n_images) and ops.rgb_reverse_form(n_images, True) == "sc_rgb_composite_backward_fused_" + form
    assert names == [("sc_rgb_composite_backward_fused_" + form, S)], names


@pytest.mark.parametrize("n_images,rpi,S", list(C.RGB_CASES))
def test_rgb_fused_reverse_float64_budget(n_images, rpi, S):
    """(a) as test_rgb_composite_float64_budget: default (sc_rgb_composite_backward_fused_split) and twins (_fused_stash) against the
    float64 restatement, rules (a) and (b) with K_RGB; fewer than 4 rays per image, up to the 256 images the fused form takes."""
    from shapeclipper_amd import ops
    (ins, Wr, zr, hit, cot), ref = _rgb_refs(n_images, rpi, S)
    assert ins["z_vals"].shape == (n_images * rpi, S)
    print("hit fraction %.2f" % float(hit.float().mean()))
    assert float(hit.float().mean()) >= 0.25
    with _reverse_entries() as names, F._count_wgrad() as calls:
        od, gd = F._rgb_hip(ins, Wr, zr, rpi, cot)
        _fused_ran(names, n_images, S, "split")
    with F._twins(), _reverse_entries() as names:
        ot, gt = F._rgb_hip(ins, Wr, zr, rpi, cot)
        _fused_ran(names, n_images, S, "stash")
    assert len(calls) == 0
    assert torch.equal(od["mask_hard"], ot["mask_hard"])
    rows = F._rgb_rows(ref, hit, od, gd, ot, gt)
    title = "RGB fused reverse n_images=%d rays/image=%d S=%d" % (n_images, rpi, S)
    _worst(title, rows, F.K_RGB)
    F._check(title, rows, F.K_RGB)


def _rgb_direct(ins, Wr, zr, rpi, cot):
    """RgbCompositeFunction forward + backward, the gradients taken at the kernel's own inputs: g_dbias [n_images, 3, 64] and the
    per-sample gradients by name, on the CPU."""
    from shapeclipper_amd import packing
    from shapeclipper_amd.functional import RgbCompositeFunction
    n_pts = ins["points"].shape[0]
    L = {k: (packing.rows_to_tbl(v) if k == "feat" else v).to(DEV).contiguous().requires_grad_(True) for k, v in ins.items()}
    v_pack, dbias = packing.pack_rgb({k: v.to(DEV).requires_grad_(True) for k, v in Wr.items()}, zr.to(DEV).requires_grad_(True))
    rgb, mask, mask_hard, depth, normal = RgbCompositeFunction.apply(L["points"], L["z_vals"], L["depth_fac"], L["sdf"], L["grad"], L["feat"],
                                                                     v_pack, dbias, L["beta"], rpi, True, 1e-4, 1.0, 1.0, False)
    o = dict(rgb=rgb, mask=mask, depth=depth, normal=normal)
    f = sum((o[k] * cot[k].to(DEV)).sum() for k in cot)
    names = ("sdf", "grad", "feat", "points", "z_vals")
    gs = torch.autograd.grad(f, [dbias] + [L[k] for k in names])
    torch.cuda.synchronize()
    out = dict(zip(names, [x.cpu() for x in gs[1:]]))
    out["feat"] = packing.tbl_to_rows(gs[1 + names.index("feat")], n_pts).cpu()
    return gs[0].cpu(), out


@pytest.mark.parametrize("n_images,rpi,S", C.RGB_LEAK_CASES)
def test_rgb_fused_reverse_leaks_nothing_into_other_images(n_images, rpi, S):
    """(b) one hot image: the g_dbias rows and the per-sample gradients (sdf, d sdf/dx, feature, points, z_vals) of every other image are
    exactly zero; image h's against the float64 oracle under the same cotangents, rules (a) and (b) with K_RGB (d L / d lin_l.bias IS
    g_dbias[h, l] then)."""
    assert S == 64
    (ins, Wr, zr, hit, cot), _ = _rgb_refs(n_images, rpi, S)
    from oracle import reference_ops as R
    cfg = R.Cfg()
    per_ray = lambda x: x.reshape(n_images, rpi, -1)
    for h in C.hot_images(n_images):
        ch = {k: torch.zeros_like(v) for k, v in cot.items()}
        for k in cot:
            ch[k][h * rpi:(h + 1) * rpi] = cot[k][h * rpi:(h + 1) * rpi]
        with _reverse_entries() as names:
            d_db, d = _rgb_direct(ins, Wr, zr, rpi, ch)
            _fused_ran(names, n_images, S, "split")
        with F._twins(), _reverse_entries() as names:
            t_db, t = _rgb_direct(ins, Wr, zr, rpi, ch)
            _fused_ran(names, n_images, S, "stash")
        other = torch.ones(n_images, dtype=torch.bool)
        other[h] = False
        for arm, db, g in (("default", d_db, d), ("twins", t_db, t)):
            assert db.shape == (n_images, 3, 64)
            bad = {"dbias": int((db[other] != 0).sum())}
            bad.update({k: int((per_ray(v)[other] != 0).sum()) for k, v in g.items()})
            assert not any(bad.values()), "%s arm, hot image %d: gradient elements of other images that are not zero: %s" % (arm, h, bad)
            assert float(db[h].abs().max()) > 0 and all(float(per_ray(v)[h].abs().max()) > 0 for v in g.values())
        _, g64 = F._rgb_oracle(cfg, ins, Wr, zr, rpi, ch, torch.float64)
        _, g32 = F._rgb_oracle(cfg, ins, Wr, zr, rpi, ch, torch.float32)
        e = F._err
        rows = {"g_dbias[%d, %d]" % (h, l): ("w_rgb", e(d_db[h, l], g64[b]), e(t_db[h, l], g64[b]), e(g32[b], g64[b]))
                for l, b in enumerate("rgb_network.lin%d.bias" % l for l in range(3))}
        rows.update({k: ("point", e(d[k], g64[k]), e(t[k], g64[k]), e(g32[k], g64[k])) for k in d})
        title = "RGB fused reverse n_images=%d rays/image=%d, hot image %d" % (n_images, rpi, h)
        _worst(title, rows, F.K_RGB)
        F._check(title, rows, F.K_RGB)
