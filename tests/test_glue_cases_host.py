"""Preconditions of the cases of tests/glue_cases.py, checked on the CPU: they make the GPU comparison of test_gpu_glue_float64.py exact
rather than "up to exclusions" (the same rays are kept by the robust normal loss in every precision, no mask sits on the 0.5 threshold,
no L1 term sits on its kink), and the references free of precision leaks (an fp32 constant inside a float64 run)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_cases as C  # noqa: E402

F32, F64 = torch.float32, torch.float64
GAP = 1e-5            # two orders above the fp32 rounding of an angular error 1 - <p, t> of unit vectors (~1e-7)


def _agree(a, b, what, tol=1e-5):
    """Every tensor of the fp32 reference within tol of max of the float64 one (NaN only where both are)."""
    for k in b:
        x, y = a[k].double(), b[k].double()
        assert x.shape == y.shape, (what, k)
        assert torch.equal(torch.isnan(x), torch.isnan(y)), (what, k)
        x, y = torch.nan_to_num(x), torch.nan_to_num(y)
        scale = float(y.abs().max()) if y.numel() else 0.0
        err = float((x - y).abs().max()) if y.numel() else 0.0
        assert err <= tol * scale, "%s %s: fp32 and float64 references differ by %.3e of max %.3e" % (what, k, err, scale)


@pytest.mark.parametrize("case", list(C.LOSS_CASES))
def test_normal_loss_keeps_the_same_rays_in_every_precision(case):
    """The gap between the float64 angular errors at ranks n_keep and n_keep + 1 is at least 1e-5.  Where exact duplicates are planted
    across that boundary, the tie group is made of planted rays only and everything else is 1e-5 away from it."""
    c = C.loss_inputs(case)
    idx, ang = C._angular64(c)
    n = len(idx)
    k = C.n_keep_of(n, c["tol"])
    order = torch.argsort(ang, stable=True)
    v = ang[order]
    print("%s: %d masked rays, n_keep %d" % (case, n, k))
    # the rays the reference keeps are the first n_keep of a stable sort; unless ties are planted, torch's own order keeps the same ones
    expect = torch.zeros(c["B"] * c["R"], dtype=torch.bool)
    expect[idx[order[:k]]] = True
    assert torch.equal(C.kept_rays(c), expect)
    plain = C.kept_rays(c, stable=False)
    if c["planted"]:
        differ = torch.nonzero(plain != expect).view(-1).tolist()
        assert set(differ) <= set(c["planted"]) and int(plain[list(c["planted"])].sum()) == 1
    else:
        assert torch.equal(plain, expect)
    if k == 0 or k == n:
        assert not c["planted"]
        return
    if not c["planted"]:
        assert float(v[k] - v[k - 1]) >= GAP, float(v[k] - v[k - 1])
        return
    planted = torch.tensor(c["planted"])
    assert len(planted) == C.N_PLANTED + 1 and bool(torch.isin(planted, idx).all())
    tie = ang[torch.isin(idx, planted)]
    assert float(tie.max() - tie.min()) == 0.0                                   # exact duplicates in float64, hence in fp32
    assert float(v[k - 1]) == float(tie[0]) and float(v[k]) == float(tie[0])     # the boundary falls inside the tie group
    assert int((v[:k] < tie[0]).sum()) == k - 1                                  # exactly one of the ties is kept ...
    kept = idx[order[:k]]
    assert int(torch.isin(kept, planted).sum()) == 1 and int(planted.min()) in kept.tolist()      # ... the one with the lowest index
    others = ang[~torch.isin(idx, planted)]
    assert float((others - tie[0]).abs().min()) >= GAP


@pytest.mark.parametrize("case", list(C.LOSS_CASES))
def test_masks_and_l1_terms_are_off_their_thresholds(case):
    c = C.loss_inputs(case)
    assert float((c["mask"] - 0.5).abs().min()) > 1e-6
    assert float((c["mask_t"] - 0.5).abs().min()) > 1e-6
    assert int((c["normal"] - c["normal_t"] == 0).sum()) == 0
    assert int((c["normal"].double() - c["normal_t"].double() == 0).sum()) == 0


def test_loss_cases_reach_what_they_are_meant_to():
    cases = C.LOSS_CASES
    assert {m for _, _, _, m, _ in cases.values()} == {0.0, 0.3} and {t for *_, t in cases.values()} == {0.0, 0.2, 0.5}
    assert any(E is None for _, _, E, _, _ in cases.values()) and any(E not in (None, n) for _, n, E, _, _ in cases.values())
    assert (16, 1024) in {(B, n) for B, n, *_ in cases.values()} and (17, 1024) in {(B, n) for B, n, *_ in cases.values()}
    c = C.loss_inputs("3x100x37")
    assert float(c["mask"][0].abs().max()) == 0.0 and float(c["mask_t"][0].abs().max()) == 0.0
    assert bool(((c["mask"][1] > 0.5) & (c["mask_t"][1] > 0.5)).all())
    idx, _ = C._angular64(C.loss_inputs("1x1x1"))
    assert len(idx) == 1 and C.n_keep_of(1, cases["1x1x1"][4]) == 0


@pytest.mark.parametrize("case", list(C.CAMERA_CASES))
def test_camera_cases_plant_the_corner_pixels(case):
    c = C.camera_inputs(case)
    B, n, H, W, sampled, _ = C.CAMERA_CASES[case]
    assert float((c["intr"][:, 0, 1]).abs().min()) > 0 and bool((c["intr"][:, 0, 0] != c["intr"][:, 1, 1]).all())
    if not sampled:
        assert c["ray_idx"] is None and n == H * W
        return
    idx = c["ray_idx"]
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (B, n) and int(idx.min()) >= 0 and int(idx.max()) < H * W
    if n >= 6:
        for b in range(B):
            row = idx[b].tolist()
            assert {0, W - 1, (H - 1) * W, H * W - 1} <= set(row) and len(set(row)) < n


@pytest.mark.parametrize("case", list(C.LOSS_CASES))
@pytest.mark.parametrize("subset", list(C.LOSS_SUBSETS))
def test_loss_references_agree(case, subset):
    r32, r64 = C.loss_reference(case, subset, F32), C.loss_reference(case, subset, F64)
    _agree(r32, r64, "loss %s %s" % (case, subset))
    for k in ("g_normal", "g_normal_t"):
        assert torch.equal(r32[k].abs().sum(-1) != 0, r64[k].abs().sum(-1) != 0), k       # the same rays are kept
    if case == "1x1x1":
        assert bool(torch.isnan(r64["normal"])) and float(r64["g_normal"].abs().max()) == 0.0


@pytest.mark.parametrize("case", list(C.CAMERA_CASES))
@pytest.mark.parametrize("subset", list(C.CAMERA_SUBSETS))
def test_camera_references_agree(case, subset):
    # the far variant cancels (R^T g + t_inv) - t_inv against t_inv ~ 50: the fp32 reference is itself 10x further from float64 there
    _agree(C.camera_reference(case, subset, F32), C.camera_reference(case, subset, F64), "camera %s %s" % (case, subset))


@pytest.mark.parametrize("B", C.TRIG_B)
@pytest.mark.parametrize("subset", list(C.TRIG_SUBSETS))
def test_trig_references_agree(B, subset):
    c = C.trig_inputs(B)
    norms = torch.cat([c["leaves"][k].norm(dim=1) for k in ("azim", "elev", "theta")])
    assert float(norms.min()) >= 0.3 - 1e-6 and float(norms.max()) <= 2.0 + 1e-6 and float((norms - 1).abs().min()) > 0
    _agree(C.trig_reference(B, subset, F32), C.trig_reference(B, subset, F64), "pose_from_trig B=%d %s" % (B, subset))


@pytest.mark.parametrize("B,n", C.NORMAL_CASES)
def test_transform_normal_references_agree(B, n):
    r64 = C.normal_reference(B, n, F64)
    assert float(r64["d_pose"][:, :, 3].abs().max()) == 0.0
    _agree(C.normal_reference(B, n, F32), r64, "transform_normal B=%d R=%d" % (B, n))


@pytest.mark.parametrize("B,Z,L,NL,with_post", C.LATENT_CASES)
def test_latent_references_agree(B, Z, L, NL, with_post):
    r64 = C.latent_reference(B, Z, L, NL, with_post, F64)
    assert tuple(r64["out"].shape) == (B, NL, 64) and tuple(r64["g_lat"].shape) == (L * 64, Z)
    c = C.latent_inputs(B, Z, L, NL, with_post)
    assert torch.equal(r64["out"][:, L:], c["bias"][L:].double().expand(B, NL - L, 64))         # zero-padded to NL
    _agree(C.latent_reference(B, Z, L, NL, with_post, F32), r64, "latent bias %s" % ((B, Z, L, NL, with_post),))


def test_chain_references_agree():
    c = C.chain_inputs()
    for k in ("azim", "elev", "theta"):
        assert float((c["leaves"][k].norm(dim=1) - 1).abs().max()) < 1e-6
    _agree(C.chain_reference(F32), C.chain_reference(F64), "chain")


def test_references_leave_the_default_dtype_alone():
    assert torch.get_default_dtype() == torch.float32
    assert C.camera_reference("1x1_8x8", "all", F64)["d_pose"].dtype == F64 and C.camera_reference("1x1_8x8", "all", F32)["d_pose"].dtype == F32
    assert torch.get_default_dtype() == torch.float32
