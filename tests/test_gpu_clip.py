"""CLIP ViT image tower (csrc/clip_vit.hip) vs transformers.CLIPVisionModelWithProjection (fp32, CPU) with
seeded random weights -- architecture-level oracle; parity with the reference is unpinned (openai/CLIP is an
un-vendored dependency of CLIP_anno.py:16 and no weights are available offline).

Arithmetic: the tower's default is IEEE fp16 operands with fp32 accumulation and fp32 LayerNorm / softmax statistics -- what the
reference's dependency runs on a GPU (clip.load(..., device="cuda"), CLIP_anno.py:16); bf16 operands are the other option.
Bars (embedding vs the fp32 architecture oracle; measured values are printed): fp16  cos > 0.99999 and max abs error < 0.4 % of
max |ref| (measured round 3: cos >= 0.9999980, <= 0.18 %, ViT-L/14 at full depth 0.9999998 / 0.07 %);  bf16  cos > 0.9999 and
< 2.5 % (measured: cos >= 0.99993, <= 1.3 %).
What the reference USES the embeddings for is a cosine k-NN (CLIP_anno.py:29-41): test_clip_knn_indices_match_fp32_oracle checks the
neighbour INDICES on a 256-image set."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _hf(width, layers, heads, mlp, patch, image, proj, seed):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(seed)
    cfg = CLIPVisionConfig(hidden_size=width, intermediate_size=mlp, num_hidden_layers=layers, num_attention_heads=heads,
                           patch_size=patch, image_size=image, projection_dim=proj, hidden_act="quick_gelu")
    m = CLIPVisionModelWithProjection(cfg).eval()
    with torch.no_grad():      # make biases / LN params non-trivial
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
            else:
                p.mul_(3.0)
    return m


BARS = {"fp16": (0.99999, 0.004), "bf16": (0.9999, 0.025)}


def _check(got, ref, dtype, what):
    cos = torch.nn.functional.cosine_similarity(got, ref, dim=-1)
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    print("CLIP tower %s, %s: min cosine %.7f, max abs error %.3f %% of max |ref|" % (what, dtype, cos.min().item(), 100 * err))
    assert torch.isfinite(got).all()
    assert cos.min().item() > BARS[dtype][0], cos
    assert err < BARS[dtype][1]


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("width,layers,heads,mlp,patch,image,proj,B", [
    (128, 2, 2, 256, 32, 64, 64, 3),             # 5 tokens
    (768, 12, 12, 3072, 32, 224, 512, 4),        # ViT-B/32: 50 tokens
    (768, 12, 12, 3072, 32, 224, 512, 32),       # ViT-B/32 at the BASELINE config[2] batch (1600 token rows: 64-wide tiles)
    (128, 2, 2, 256, 14, 112, 64, 2),            # 65 tokens (> one key chunk... and 2 query blocks + 1), patch K = 588 (padded)
    (192, 2, 3, 384, 8, 112, 96, 2),             # 197 tokens: 7 key chunks, query blocks wrap over the 4 waves
    (1024, 2, 16, 4096, 14, 224, 768, 2),        # ViT-L/14 geometry (257 tokens), 2 layers
    (128, 2, 2, 256, 13, 221, 64, 2),            # 290 tokens: ten query blocks, no key split (a wave walks two query blocks); K = 507 (padded)
    (128, 2, 2, 256, 16, 368, 64, 2),            # 530 tokens: key split with 18 left-over queries, three key chunks for wave 0
    (128, 2, 2, 256, 14, 336, 64, 2),            # 577 tokens (ViT-L/14@336px): K no longer fits LDS, read from global memory in both passes
])
def test_clip_tower_vs_transformers(width, layers, heads, mlp, patch, image, proj, B, dtype):
    from shapeclipper_amd.model.clip_vit import ClipVisionTower
    hf = _hf(width, layers, heads, mlp, patch, image, proj, seed=width)
    x = torch.randn(B, 3, image, image)
    with torch.no_grad():
        ref = hf(pixel_values=x).image_embeds
    tower = ClipVisionTower(image_size=image, patch=patch, width=width, layers=layers, heads=heads, mlp=mlp, proj=proj, dtype=dtype)
    tower.load_state_dict(hf.state_dict())
    tower = tower.cuda()
    got = tower.encode_image(x.cuda()).cpu()
    _check(got, ref, dtype, "%d x %d layers, patch %d, B=%d" % (width, layers, patch, B))


def test_clip_vit_l14_full_depth():
    """The model the reference loads (CLIP_anno.py:16): ViT-L/14, all 24 layers, 257 tokens, in its own fp16 arithmetic."""
    import os
    from shapeclipper_amd.model.clip_vit import VIT_L14, ClipVisionTower
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    hf = _hf(1024, 24, 16, 4096, 14, 224, 768, seed=14)
    x = torch.randn(2, 3, 224, 224)
    with torch.no_grad():
        ref = hf(pixel_values=x).image_embeds
    tower = ClipVisionTower(**VIT_L14)
    assert tower.dtype16 == "fp16"
    tower.load_state_dict(hf.state_dict())
    got = tower.cuda().encode_image(x.cuda()).cpu()
    _check(got, ref, "fp16", "ViT-L/14, 24 layers, B=2")


def test_clip_knn_indices_match_fp32_oracle():
    """The reference uses the tower for ONE thing: L2-normalise the embeddings, cosine similarity of all pairs, top-k (CLIP_anno.py:
    29-41,166-167).  256 synthetic images in 32 loose clusters, ViT-B/32: the neighbour lists computed from the HIP fp16 embeddings
    must equal those computed from the fp32 architecture oracle's embeddings -- position by position, except where the oracle's own
    similarities of two adjacent candidates are closer than 4x the largest similarity error (a genuine near-tie; counted, printed)."""
    import os
    from shapeclipper_amd.model.clip_vit import VIT_B32, ClipVisionTower
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    hf = _hf(768, 12, 12, 3072, 32, 224, 512, seed=7)
    g = torch.Generator().manual_seed(3)
    centres = torch.randn(32, 3, 224, 224, generator=g)
    imgs = (centres[:, None] + 0.6 * torch.randn(32, 8, 3, 224, 224, generator=g)).reshape(256, 3, 224, 224)
    with torch.no_grad():
        ref = torch.cat([hf(pixel_values=imgs[i:i + 32]).image_embeds for i in range(0, 256, 32)])
    tower = ClipVisionTower(**VIT_B32)
    tower.load_state_dict(hf.state_dict())
    tower = tower.cuda()
    got = torch.cat([tower.encode_image(imgs[i:i + 32].cuda()) for i in range(0, 256, 32)]).cpu()
    k = 6                                            # options/clip/pix3d.yaml: k_nearest
    nrm = lambda e: torch.nn.functional.normalize(e.double(), dim=-1)
    s_ref, s_got = nrm(ref) @ nrm(ref).t(), nrm(got) @ nrm(got).t()
    sim_err = float((s_ref - s_got).abs().max())
    v_ref, i_ref = s_ref.topk(k + 1, dim=1)
    _, i_got = s_got.topk(k, dim=1)
    exact = (i_ref[:, :k] == i_got)
    gaps = (v_ref[:, :-1] - v_ref[:, 1:])            # oracle gap between candidate j and j + 1
    near_tie = torch.zeros_like(exact)
    near_tie[:, 1:] |= gaps[:, :k - 1] < 4 * sim_err
    near_tie |= gaps[:, :k] < 4 * sim_err
    bad = ~exact & ~near_tie
    print("CLIP k-NN on 256 images: %d / %d neighbour positions identical, %d differ at oracle near-ties (< %.1e), %d wrong; "
          "max |cos_hip - cos_fp32| %.2e, smallest / median top-%d gap %.2e / %.2e"
          % (int(exact.sum()), exact.numel(), int((~exact & near_tie).sum()), 4 * sim_err, int(bad.sum()), sim_err, k,
             float(gaps[:, :k].min()), float(gaps[:, :k].median())))
    assert (i_got[:, 0] == torch.arange(256)).all()             # a query's first neighbour is itself
    assert not bad.any()
    assert exact.float().mean() > 0.97


def _gemm_plan(epi, M, N, K):
    """"main kernel[+tail kernel]" of the plan sc_gemm_plan reports for this device: the kernel a GEMM test runs is asserted, not assumed"""
    import ctypes
    from shapeclipper_amd import _lib
    out = (ctypes.c_int * 5)()
    assert _lib.load().sc_gemm_plan(epi, M, N, K, 0, out) == 0
    main = ("t64", "t128", "persist", "gemm8p", "gemm8p_192", "gemm256")[out[0]]
    return main + ("", "+thin", "+t64")[out[2]]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("M,N,K", [(200, 192, 128), (1600, 768, 768), (12800, 2304, 768)])       # 12 / 300 tiles of 64 x 64; 450 tiles of 256 x 256 (csrc/gemm8p.hpp)
def test_gemm_16bit_transpose_detecting(M, N, K, dtype):
    """C = A W^T with asymmetric operands (catches swapped row/col in the MFMA C/D mapping); the 16-bit operands are exact inputs,
    so the only error is the fp32 accumulation order."""
    import ctypes
    from shapeclipper_amd import _lib
    lib = _lib.load()
    assert _gemm_plan(0, M, N, K) == {200: "t64", 1600: "t64", 12800: "gemm8p"}[M]
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    td = torch.bfloat16 if dtype == "bf16" else torch.float16
    A = torch.randn(M, K, device=dev).to(td)
    W = (torch.randn(N, K, device=dev) + torch.arange(N, device=dev)[:, None] * 0.01).to(td)
    bias = torch.randn(N, device=dev)
    out = torch.zeros(M, N, device=dev)
    fn = lib.sc_gemm_bf16 if dtype == "bf16" else lib.sc_gemm_f16
    rc = fn(ctypes.c_int(0), _lib.ptr(A), _lib.ptr(W), _lib.ptr(bias), _lib.ptr(out), ctypes.c_int(M), ctypes.c_int(N), ctypes.c_int(K),
            _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    ref = (A.double() @ W.double().t() + bias.double()).float()
    assert (out - ref).abs().max().item() < 1e-5 * ref.abs().max().item()


GEMM_PLANS = {          # per epilogue 0..3, on 256 CUs
    (12800, 768, 3072): ("gemm8p_192", "gemm8p_192", "persist+t64", "persist+t64"),
    (8224, 1024, 1024): ("persist+thin",) * 4,
    (2049, 256, 64): ("t64",) * 4,
    (12800, 3072, 768): ("gemm8p",) * 4,
    (8224, 3072, 1024): ("gemm8p",) * 4,
    (8288, 1024, 4096): ("persist+thin",) * 4,
    (8224, 4096, 1024): ("gemm8p+thin",) * 4,
    (2049, 6144, 64): ("gemm8p",) * 4,
    (4100, 3328, 192): ("gemm8p",) * 4,
}


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("M,N,K", [(12800, 768, 3072), (8224, 1024, 1024), (2049, 256, 64), (12800, 3072, 768),
                                   (8224, 3072, 1024), (8288, 1024, 4096), (8224, 4096, 1024),
                                   (2049, 6144, 64), (4100, 3328, 192)])     # gemm8p with ONE / three K-tiles per output tile and one / four valid rows in the last row tile
def test_gemm_256_tiles_all_epilogues(M, N, K, dtype):
    """Round 4: shapes with >= 200 tiles of 256 x 256 (12800 x 3072, 8224 x 3072 / 4096, the last two) run on csrc/gemm8p.hpp -- hand-counted
    vmcnt, residual tile as accumulator init, paired 16-byte 16-bit stores through a buffer resource that ends at row M (tools/micro/gemm_lab
    `stress` is its race screen: profiles/r04_gemm_stress.txt); 8224 x 4096 with its 32 ragged rows peeled off into gemm_thin_kernel.
    12800 x 768: the 256 x 192 form of gemm8p for the fp32 epilogues, the persistent 128 x 128 kernel with a 64-wide tail for the 16-bit
    ones.  8224 / 8288 x 1024: the persistent 128 x 128 kernel with its ragged last rows peeled off into gemm_thin_kernel (8224 = 64 x 128
    + 32 rows: ViT-L/14 at batch 32; 8288: 96 rows).  2049 x 256: 64 x 64 tiles.  (gemm256_kernel runs for none of them: GEMM_PLANS, asserted
    below.)  Every epilogue (fp32, residual accumulate, QuickGELU -> 16 bit, 16 bit) against float64; the residual epilogue must read its
    rows before it writes them, nothing is written past row M."""
    import ctypes
    from shapeclipper_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(M + N)
    td = torch.bfloat16 if dtype == "bf16" else torch.float16
    A = (torch.randn(M, K, device=dev) * 0.5).to(td)
    W = ((torch.randn(N, K, device=dev) + torch.arange(N, device=dev)[:, None] * 0.002) * 0.1).to(td)
    bias = torch.randn(N, device=dev)
    fn = lib.sc_gemm_bf16 if dtype == "bf16" else lib.sc_gemm_f16
    ref = A.double() @ W.double().t() + bias.double()
    scale = ref.abs().max().item()
    resid = torch.randn(M, N, device=dev)
    for epi in (0, 1, 2, 3):
        assert _gemm_plan(epi, M, N, K) == GEMM_PLANS[M, N, K][epi]
        if epi == 1:
            out = resid.clone()
            want = ref + resid.double()
        elif epi == 2:
            out = torch.zeros(M, N, device=dev, dtype=td)
            want = ref * torch.sigmoid(1.702 * ref)
        else:
            out = torch.zeros(M, N, device=dev, dtype=torch.float32 if epi == 0 else td)
            want = ref
        pad = torch.full((4096,), 7.0, device=dev, dtype=out.dtype)          # a canary behind the output: the ragged tile must not write past row M
        buf = torch.cat([out.view(-1), pad]); out = buf[:M * N].view(M, N)
        rc = fn(ctypes.c_int(epi), _lib.ptr(A), _lib.ptr(W), _lib.ptr(bias), _lib.ptr(out), ctypes.c_int(M), ctypes.c_int(N), ctypes.c_int(K), _lib.stream())
        assert rc == 0
        torch.cuda.synchronize()
        tol = 1e-5 if epi in (0, 1) else (8e-3 if dtype == "bf16" else 1e-3)
        err = (out.double() - want).abs().max().item()
        assert err < tol * max(scale, 1.0), (epi, err, scale)
        assert (buf[M * N:] == 7.0).all()


def test_clip_tower_golden_fixture():
    """G11 (tests/golden/make_golden_clip.py): committed weights / input / embedding of a shrunken tower."""
    import os
    from shapeclipper_amd.model.clip_vit import ClipVisionTower
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "g11_clip_arch.npz"))
    width, layers, heads, mlp, patch, image, proj = (int(v) for v in g["cfg"])
    tower = ClipVisionTower(image_size=image, patch=patch, width=width, layers=layers, heads=heads, mlp=mlp, proj=proj)
    tower.load_state_dict({k[2:]: torch.tensor(g[k]) for k in g.files if k.startswith("w.")})
    got = tower.cuda().encode_image(torch.tensor(g["input"]).cuda()).cpu()
    _check(got, torch.tensor(g["embedding"]), "fp16", "G11 fixture")


@pytest.mark.parametrize("res,patch,width,layers,proj,B", [
    (224, 32, 768, 12, 512, 4),          # ViT-B/32, full depth
    (224, 14, 1024, 2, 768, 2),          # ViT-L/14 geometry (the reference's model, CLIP_anno.py:16), 2 layers
])
def test_clip_tower_from_openai_state_dict(res, patch, width, layers, proj, B):
    """VERDICT r04 next #6a: the REAL-checkpoint entry point.  A state dict in openai/CLIP's own naming and storage (fp16 weights, fp32
    LayerNorm, packed attn.in_proj_weight, [width, out] visual.proj: oracle/clip_openai_ref.py, torch's nn.MultiheadAttention) goes through
    ClipVisionTower.from_openai_state_dict with the geometry inferred from its shapes; the HIP embeddings must match the original-architecture
    forward evaluated in fp32 on the same (fp16-rounded) weights at the tower's usual bars."""
    from oracle import clip_openai_ref as O
    from shapeclipper_amd.model.clip_vit import ClipVisionTower
    ref_model, sd16 = O.seeded(res, patch, width, layers, proj, seed=width + layers, fp16_storage=True)
    ref_model.load_state_dict({k: v.float() for k, v in sd16.items()})          # the oracle computes in fp32 on the SAME stored values
    x = torch.randn(B, 3, res, res)
    with torch.no_grad():
        ref = ref_model.encode_image(x)
    tower = ClipVisionTower.from_openai_state_dict(sd16).cuda()
    assert tower.cfg["heads"] == width // 64 and tower.cfg["layers"] == layers and tower.cfg["proj"] == proj
    _check(tower.encode_image(x.cuda()).cpu(), ref, "fp16", "from openai names, %d x %d layers, patch %d" % (width, layers, patch))


# ---- the small-batch cluster form of the ViT-B layers (csrc/clip_cluster.hpp) -----------------------------------------------------------
def _cluster_range(lo, hi):
    import ctypes
    from shapeclipper_amd import _lib
    _lib.check(_lib.load().sc_clip_cluster_set_batch_range(ctypes.c_int(lo), ctypes.c_int(hi)), "sc_clip_cluster_set_batch_range")


@pytest.fixture
def cluster_range():
    """Tests move the batch range of the cluster form; the default (26..32) is restored afterwards."""
    yield _cluster_range
    _cluster_range(26, 32)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("B", [1, 7, 32, 41])            # one image; a ragged last group of 8; the BASELINE batch; a second round of the chip
def test_clip_cluster_form_vs_transformers_and_launch_form(B, dtype, cluster_range):
    """Both forms of the tower against the fp32 architecture oracle at the bars above, and against each other: they differ only in the
    summation order of the K-partials and of the LayerNorm sums (cos > 0.999999 between them; bf16: 0.9999)."""
    from shapeclipper_amd.model.clip_vit import ClipVisionTower, VIT_B32
    c = VIT_B32
    hf = _hf(c["width"], c["layers"], c["heads"], c["mlp"], c["patch"], c["image_size"], c["proj"], seed=11)
    x = torch.randn(B, 3, 224, 224)
    with torch.no_grad():
        ref = hf(pixel_values=x).image_embeds
    tower = ClipVisionTower(**c, dtype=dtype)
    tower.load_state_dict(hf.state_dict())
    tower = tower.cuda()
    cluster_range(1, 64)
    got_c = tower.encode_image(x.cuda()).cpu()
    again = tower.encode_image(x.cuda()).cpu()
    cluster_range(1, 0)                                   # never
    got_l = tower.encode_image(x.cuda()).cpu()
    _check(got_c, ref, dtype, "ViT-B/32 cluster form, B=%d" % B)
    _check(got_l, ref, dtype, "ViT-B/32 launch form, B=%d" % B)
    assert torch.equal(got_c, again), "the cluster form is deterministic (fixed summation order, no atomics in the data path)"
    assert not torch.equal(got_c, got_l), "both calls ran the same form: the batch range did not take effect"
    cos = torch.nn.functional.cosine_similarity(got_c, got_l, dim=-1).min().item()
    print("cluster form vs launch form, %s, B=%d: min cosine %.8f, max |diff| %.2e" % (dtype, B, cos, (got_c - got_l).abs().max().item()))
    assert cos > (0.999999 if dtype == "fp16" else 0.9999)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("image", [160, 192])            # 26 tokens (one key chunk, masked) and 37 (two chunks): ViT-B/32 runs 50
def test_clip_cluster_form_vs_launch_form_at_other_token_counts(image, dtype, cluster_range):
    """The cluster form at token counts other than ViT-B/32's 50, B = 2 with the batch range opened: both forms against the fp32
    architecture oracle at the tower's bars and against each other at the bars of the test above."""
    from shapeclipper_amd.model.clip_vit import ClipVisionTower, VIT_B32
    c = dict(VIT_B32, image_size=image)
    hf = _hf(c["width"], c["layers"], c["heads"], c["mlp"], c["patch"], image, c["proj"], seed=image)
    x = torch.randn(2, 3, image, image)
    with torch.no_grad():
        ref = hf(pixel_values=x).image_embeds
    tower = ClipVisionTower(**c, dtype=dtype)
    tower.load_state_dict(hf.state_dict())
    tower = tower.cuda()
    cluster_range(1, 64)
    got_c = tower.encode_image(x.cuda()).cpu()
    again = tower.encode_image(x.cuda()).cpu()
    cluster_range(1, 0)                                   # never
    got_l = tower.encode_image(x.cuda()).cpu()
    T = (image // 32) ** 2 + 1
    _check(got_c, ref, dtype, "ViT-B width, %d tokens, cluster form" % T)
    _check(got_l, ref, dtype, "ViT-B width, %d tokens, launch form" % T)
    assert torch.equal(got_c, again)
    assert not torch.equal(got_c, got_l), "both calls ran the same form: the batch range did not take effect"
    cos = torch.nn.functional.cosine_similarity(got_c, got_l, dim=-1).min().item()
    print("cluster form vs launch form, %s, %d tokens: min cosine %.8f, max |diff| %.2e" % (dtype, T, cos, (got_c - got_l).abs().max().item()))
    assert cos > (0.999999 if dtype == "fp16" else 0.9999)


def test_clip_cluster_form_is_batch_invariant(cluster_range):
    """An image is owned by one cluster whatever else is in the batch: row i of a batch of 32 is bit-identical to the image run alone."""
    from shapeclipper_amd.model.clip_vit import ClipVisionTower, VIT_B32
    torch.manual_seed(5)
    tower = ClipVisionTower(**VIT_B32).cuda()
    x = torch.randn(32, 3, 224, 224, device="cuda")
    cluster_range(1, 64)
    full = tower.encode_image(x)
    for i in (0, 13, 31):
        assert torch.equal(tower.encode_image(x[i:i + 1])[0], full[i]), i
    # ... and the default range takes the BASELINE batch through the cluster form
    cluster_range(26, 32)
    assert torch.equal(tower.encode_image(x), full)
