"""dist_chamfer_3D on the GPU: the forward is chamfer_3D.forward's, the gradient is the definition's within a derived fp32 bound, and the
ordered backward (csrc/chamfer_bwd.hip) has the same bits whatever the run, the batch, the stream or the reserved-CU setting.

The bound (tests 2, 3 and 7): the term of a source is t = (2 g) * (a - b): 2 g is exact, the subtraction and the product round once each;
summing the k terms that land on a row in ANY order adds at most k - 1 roundings, +4 covers the second-order terms.  So for every output
component |hip - exact| <= (k + 4) * 2^-24 * S with S the sum of the terms' absolute values.  It is derived, not measured."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(1, 1, 1), (2, 17, 5), (3, 1000, 2049), (1, 4097, 1023), (2, 2048, 2048)]
DEV = "cuda:0"


def uniform_case(B, N, M, seed=None):
    rng = np.random.RandomState(N * 7 + M if seed is None else seed)
    a = rng.uniform(-0.5, 0.5, (B, N, 3)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, (B, M, 3)).astype(np.float32)
    gd1, gd2 = rng.standard_normal((B, N)).astype(np.float32), rng.standard_normal((B, M)).astype(np.float32)
    return tuple(torch.tensor(x, device=DEV) for x in (a, b, gd1, gd2))


def hub_case(B, seed=3):
    """50,000 points whose nearest neighbour is target 0 of a 4,096-point cloud; the other 4,095 targets are far away."""
    rng = np.random.RandomState(seed)
    a = rng.uniform(-0.01, 0.01, (B, 50000, 3)).astype(np.float32)
    b = rng.uniform(5.0, 6.0, (B, 4096, 3)).astype(np.float32)
    b[:, 0] = 0.0
    gd1, gd2 = rng.standard_normal((B, 50000)).astype(np.float32), rng.standard_normal((B, 4096)).astype(np.float32)
    return tuple(torch.tensor(x, device=DEV) for x in (a, b, gd1, gd2))


def run(x1, x2, gd1, gd2, want=(True, True)):
    """-> (g1, g2, idx1, idx2) through chamfer_3DFunction; a gradient that is not wanted comes back as None."""
    import dist_chamfer_3D
    a, b = x1.clone().requires_grad_(want[0]), x2.clone().requires_grad_(want[1])
    d1, d2, i1, i2 = dist_chamfer_3D.chamfer_3DFunction.apply(a, b)
    torch.autograd.backward([d1, d2], [gd1, gd2])
    torch.cuda.synchronize()
    return a.grad, b.grad, i1, i2


def exact(x1, x2, gd1, gd2, i1, i2):
    """float64 statement of the definition with the indices held fixed -> g1, g2, and per row the bound's k and S."""
    x1, x2, gd1, gd2 = (t.detach().cpu().numpy().astype(np.float64) for t in (x1, x2, gd1, gd2))
    i1, i2 = i1.cpu().numpy().astype(np.int64), i2.cpu().numpy().astype(np.int64)
    out = []
    for own, oth, g_own, g_oth, i_own, i_oth in ((x1, x2, gd1, gd2, i1, i2), (x2, x1, gd2, gd1, i2, i1)):
        G, S, K = np.zeros_like(own), np.zeros_like(own), np.zeros(own.shape[:2])
        for b in range(own.shape[0]):
            t_own = 2 * g_own[b][:, None] * (own[b] - oth[b][i_own[b]])
            t_oth = 2 * g_oth[b][:, None] * (oth[b] - own[b][i_oth[b]])
            G[b], S[b] = t_own, np.abs(t_own)
            np.add.at(G[b], i_oth[b], -t_oth)
            np.add.at(S[b], i_oth[b], np.abs(t_oth))
            K[b] = 1 + np.bincount(i_oth[b], minlength=own.shape[1])
        out.append((G, S, K))
    return out


def assert_within_bound(got, ref, S, K, what):
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - ref)
    bound = (K[..., None] + 4) * 2.0 ** -24 * S
    ratio = float((err / np.where(bound > 0, bound, 1.0)).max()) if err.size else 0.0
    print("%s: worst error / bound = %.3f (rows with most terms: %d)" % (what, ratio, int(K.max()) if K.size else 0))
    assert np.all(err <= bound), "%s: worst error / bound = %.3f" % (what, ratio)


# ---- 1. forward identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,M", SIZES)
def test_forward_is_chamfer_3D_forward(B, N, M):
    import chamfer_3D
    import dist_chamfer_3D
    x1, x2, _, _ = uniform_case(B, N, M)
    d1 = torch.zeros(B, N, device=DEV); d2 = torch.zeros(B, M, device=DEV)
    i1 = torch.zeros(B, N, dtype=torch.int32, device=DEV); i2 = torch.zeros(B, M, dtype=torch.int32, device=DEV)
    chamfer_3D.forward(x1, x2, d1, d2, i1, i2)
    for f in (dist_chamfer_3D.chamfer_3DFunction.apply, dist_chamfer_3D.chamfer_3DDist()):
        out = f(x1, x2)
        assert len(out) == 4 and out[2].dtype == torch.int32
        for got, want in zip(out, (d1, d2, i1, i2)):
            assert torch.equal(got, want)


# ---- 2. gradient against float64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SIZES + [(1, 100000, 100000), "hub"], ids=str)
@pytest.mark.parametrize("mode", ["ordered", "atomic"])
def test_gradient_against_float64(case, mode, monkeypatch):
    import dist_chamfer_3D
    monkeypatch.setattr(dist_chamfer_3D, "BACKWARD", mode)
    x1, x2, gd1, gd2 = hub_case(1) if case == "hub" else uniform_case(*case)
    g1, g2, i1, i2 = run(x1, x2, gd1, gd2)
    if case == "hub":
        assert bool((i1 == 0).all())                      # 50,000 terms land on row 0 of cloud 2
    (r1, s1, k1), (r2, s2, k2) = exact(x1, x2, gd1, gd2, i1, i2)
    assert_within_bound(g1, r1, s1, k1, "%s %s gradxyz1" % (case, mode))
    assert_within_bound(g2, r2, s2, k2, "%s %s gradxyz2" % (case, mode))


# ---- 3. against the oracle ----------------------------------------------------------------------------------------------------------
def _oracle_check(x1, x2, gd1, gd2, mode, monkeypatch, what):
    import dist_chamfer_3D
    from oracle import chamfer_ref
    monkeypatch.setattr(dist_chamfer_3D, "BACKWARD", mode)
    g1, g2, i1, i2 = run(x1, x2, gd1, gd2)
    o1, o2 = chamfer_ref.chamfer_backward(*(t.cpu().numpy() for t in (x1, x2, gd1, gd2, i1, i2)))
    (_, s1, k1), (_, s2, k2) = exact(x1, x2, gd1, gd2, i1, i2)
    assert_within_bound(g1, o1.astype(np.float64), s1, k1, "%s %s gradxyz1 vs oracle" % (what, mode))
    assert_within_bound(g2, o2.astype(np.float64), s2, k2, "%s %s gradxyz2 vs oracle" % (what, mode))
    return g1, g2, i1, i2


@pytest.mark.parametrize("mode", ["ordered", "atomic"])
def test_golden_with_ties_against_oracle(golden, mode, monkeypatch):
    g = golden("g9_chamfer")
    t = lambda k: torch.tensor(g[k], device=DEV)
    g1, g2, i1, i2 = _oracle_check(t("xyz1"), t("xyz2"), t("gd1"), t("gd2"), mode, monkeypatch, "g9_chamfer")
    assert np.array_equal(i1.cpu().numpy(), g["idx1"]) and np.array_equal(i2.cpu().numpy(), g["idx2"])
    (_, s1, k1), (_, s2, k2) = exact(t("xyz1"), t("xyz2"), t("gd1"), t("gd2"), i1, i2)
    assert_within_bound(g1, g["g1"].astype(np.float64), s1, k1, "g9_chamfer %s gradxyz1 vs golden" % mode)
    assert_within_bound(g2, g["g2"].astype(np.float64), s2, k2, "g9_chamfer %s gradxyz2 vs golden" % mode)


@pytest.mark.parametrize("B,N,M", [(2, 1500, 37), (3, 333, 2100)])
@pytest.mark.parametrize("mode", ["ordered", "atomic"])
def test_ragged_against_oracle(B, N, M, mode, monkeypatch):
    _oracle_check(*uniform_case(B, N, M, seed=N + M), mode, monkeypatch, "%dx%dx%d" % (B, N, M))


# ---- 4. bitwise reproducibility ------------------------------------------------------------------------------------------------------
def _case(name, B):
    return hub_case(B) if name == "hub" else uniform_case(B, 100000, 100000, seed=11)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("name", ["uniform", "hub"])
def test_five_backward_passes_have_the_same_bits(name):
    inp = _case(name, 2)
    first = run(*inp)
    for _ in range(4):
        assert _same(run(*inp), first)


@pytest.mark.parametrize("name", ["uniform", "hub"])
def test_batch_item_has_the_bits_of_the_pair_alone(name):
    inp = _case(name, 4)
    g1, g2, _, _ = run(*inp)
    for b in range(4):
        a1, a2, _, _ = run(*(t[b:b + 1].contiguous() for t in inp))
        assert torch.equal(a1[0], g1[b]) and torch.equal(a2[0], g2[b]), b


@pytest.mark.parametrize("name", ["uniform", "hub"])
def test_bits_do_not_depend_on_reserved_cus(name):
    from shapeclipper_amd import _lib
    lib = _lib.load()
    inp = _case(name, 2)
    first = run(*inp)
    try:
        lib.sc_set_reserved_cus(16)
        assert _same(run(*inp), first)
    finally:
        lib.sc_set_reserved_cus(0)


@pytest.mark.parametrize("name", ["uniform", "hub"])
def test_bits_do_not_depend_on_the_stream(name):
    inp = _case(name, 2)
    first = run(*inp)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() != torch.cuda.default_stream()
        other = run(*inp)
    side.synchronize()
    assert _same(other, first)


@pytest.mark.parametrize("B,N,M", [(2, 17, 5), (1, 3000, 11), (2, 700, 1500)])
def test_bits_are_the_headers_summation_order_restated_on_the_host(B, N, M):
    """include/shapeclipper_hip.h states the order; numpy's fp32 arithmetic (one rounding per operation) restates it here."""
    from shapeclipper_amd import _lib
    C = _lib.load().sc_chamfer3d_backward_ordered_chunk()
    x1, x2, gd1, gd2 = uniform_case(B, N, M)
    g1, g2, i1, i2 = run(x1, x2, gd1, gd2)
    f32 = np.float32
    X1, X2, G1, G2 = (t.cpu().numpy() for t in (x1, x2, gd1, gd2))
    I1, I2 = i1.cpu().numpy(), i2.cpu().numpy()
    for b in range(B):
        t1 = (f32(2) * G1[b])[:, None] * (X1[b] - X2[b][I1[b]])
        t2 = (f32(2) * G2[b])[:, None] * (X2[b] - X1[b][I2[b]])
        for own, oth, idx, got in ((t1, t2, I2[b], g1[b]), (t2, t1, I1[b], g2[b])):
            want = np.empty_like(own)
            for row in range(own.shape[0]):
                src = np.nonzero(idx == row)[0]                          # ascending source index
                S = np.zeros(3, f32)
                for c0 in range(0, len(src), C):
                    P = np.zeros(3, f32)
                    for i in src[c0:c0 + C]:
                        P = P + (-oth[i])
                    S = S + P
                want[row] = own[row] + S
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---- 5. autograd surface ----------------------------------------------------------------------------------------------------------
def test_backward_fills_both_leaves():
    import dist_chamfer_3D
    x1, x2, _, _ = uniform_case(2, 700, 900)
    a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
    d1, d2, i1, i2 = dist_chamfer_3D.chamfer_3DDist()(a, b)
    assert not i1.requires_grad and not i2.requires_grad and d1.requires_grad
    (d1.mean() + d2.mean()).backward()
    assert a.grad is not None and b.grad is not None and a.grad.shape == a.shape and b.grad.shape == b.shape
    assert float(a.grad.abs().sum()) > 0 and float(b.grad.abs().sum()) > 0


@pytest.mark.parametrize("mode", ["ordered", "atomic"])
def test_only_the_wanted_gradient_is_formed(mode, monkeypatch):
    import dist_chamfer_3D
    monkeypatch.setattr(dist_chamfer_3D, "BACKWARD", mode)
    inp = uniform_case(2, 3000, 500)
    both = run(*inp)
    g1, g2, _, _ = run(*inp, want=(True, False))
    assert g2 is None
    if mode == "ordered":
        assert torch.equal(g1, both[0])
        h1, h2, _, _ = run(*inp, want=(False, True))
        assert h1 is None and torch.equal(h2, both[1])


def test_non_contiguous_input_gives_the_bits_of_its_copy():
    x1, x2, gd1, gd2 = uniform_case(2, 1200, 800)
    wide = torch.zeros(2, 1200, 6, device=DEV)
    wide[..., ::2] = x1
    view = wide[..., ::2]
    assert not view.is_contiguous()
    g_view = run(view, x2, gd1, gd2)
    assert _same(g_view, run(x1, x2, gd1, gd2))


def test_double_backward_raises():
    import dist_chamfer_3D
    x1, x2, _, _ = uniform_case(1, 300, 200)
    a = x1.clone().requires_grad_(True)
    d1, d2, _, _ = dist_chamfer_3D.chamfer_3DFunction.apply(a, x2)
    g, = torch.autograd.grad(d1.sum() + d2.sum(), a, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


@pytest.mark.parametrize("mode", ["ordered", "atomic"])
def test_empty_cloud_gives_zero_gradients(mode, monkeypatch):
    import dist_chamfer_3D
    monkeypatch.setattr(dist_chamfer_3D, "BACKWARD", mode)
    a = torch.zeros(1, 0, 3, device=DEV, requires_grad=True)
    b = torch.rand(1, 8, 3, device=DEV).requires_grad_(True)
    d1, d2, i1, i2 = dist_chamfer_3D.chamfer_3DFunction.apply(a, b)
    assert d1.shape == (1, 0) and i1.shape == (1, 0) and bool((d2 == 0).all())
    (d1.sum() + d2.sum()).backward()
    torch.cuda.synchronize()
    assert a.grad.shape == (1, 0, 3) and b.grad.shape == (1, 8, 3) and bool((b.grad == 0).all())


# ---- 6. it descends ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_one_gradient_step_lowers_the_loss(seed):
    import dist_chamfer_3D
    N = 2048
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x1 = torch.rand(1, N, 3, device=DEV, generator=gen) - 0.5
    x2 = torch.rand(1, N, 3, device=DEV, generator=gen) - 0.5
    loss = lambda p: (lambda d: d[0].mean() + d[1].mean())(dist_chamfer_3D.chamfer_3DFunction.apply(p, x2))
    a = x1.clone().requires_grad_(True)
    before = loss(a)
    before.backward()
    with torch.no_grad():
        after = loss(x1 - 0.025 * N * a.grad)
    before, after = before.item(), after.item()
    print("seed %d: loss %.6e -> %.6e" % (seed, before, after))
    assert after < before


# ---- 7. the C ABI directly ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,M", [(2, 5000, 300), (2, 5000, 7), (1, 9, 4000)])
def test_cabi_workspace_guards_and_overwrite(B, N, M):
    from shapeclipper_amd import _lib
    lib = _lib.load()
    x1, x2, gd1, gd2 = uniform_case(B, N, M)
    g1, g2, i1, i2 = run(x1, x2, gd1, gd2)
    size = lib.sc_chamfer3d_backward_ordered_workspace_bytes(B, N, M)
    G = 4096
    for with_g2 in (True, False):
        buf = torch.full((G + size + G,), 0xA5, dtype=torch.uint8, device=DEV)
        o1 = torch.full((B, N, 3), float("nan"), device=DEV)
        o2 = torch.full((B, M, 3), float("nan"), device=DEV)
        code = lib.sc_chamfer3d_backward_ordered(_lib.ptr(x1), _lib.ptr(x2), _lib.ptr(o1), _lib.ptr(o2) if with_g2 else None, _lib.ptr(gd1),
                                                 _lib.ptr(gd2), _lib.ptr(i1), _lib.ptr(i2), B, N, M,
                                                 ctypes.c_void_p(buf.data_ptr() + G), _lib.stream())
        assert code == 0
        torch.cuda.synchronize()
        assert bool((buf[:G] == 0xA5).all()) and bool((buf[G + size:] == 0xA5).all())
        assert not bool(torch.isnan(o1).any()) and torch.equal(o1, g1)
        if with_g2:
            assert not bool(torch.isnan(o2).any()) and torch.equal(o2, g2)
        else:
            assert bool(torch.isnan(o2).all())                       # not passed: not touched
    (r1, s1, k1), (r2, s2, k2) = exact(x1, x2, gd1, gd2, i1, i2)
    assert_within_bound(g1, r1, s1, k1, "C ABI gradxyz1")
    assert_within_bound(g2, r2, s2, k2, "C ABI gradxyz2")
