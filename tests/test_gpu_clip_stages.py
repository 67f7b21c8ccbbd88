"""The stages of the CLIP image tower (csrc/clip_vit.hip) one kernel at a time against float64 (tests/clip_ref.py), through the two entry
points the tower itself launches its attention and LayerNorm with (sc_clip_attention, sc_clip_layernorm), and the embedding stages
through a zero-layer tower.  tests/test_gpu_clip.py sees these kernels only through encode_image at a cosine bar; here every branch of the
launch rule runs on inputs built so that a wrong key index, one padded key in the softmax or a slightly wrong variance is an error far
outside the bar.

Shapes: two images (the batch stride is live) x two heads (the head offset is live), width 128.  Token counts T and the branch each must
take (asserted from a restatement of the launch rule, `_branch`):

    1, 5, 32     attention_kernel, one query block, K in LDS; 32: no masked tail pass
    33, 50, 64   attention_small_kernel (both key chunks in registers)
    65           attention_kernel again, three query blocks
    256          eight query blocks, Tfull == T: no masked tail
    257          nine query blocks: key split, ONE left-over query, wave 0 alone owns a second chunk with a single valid key
    290          ten query blocks, no key split: waves 0 and 1 walk two query blocks
    530          seventeen query blocks: key split with 18 left-over queries, two or three chunks per wave, the masked chunk is the
                 last of wave 0's three
    577          K no longer fits LDS beside V^T (272 * 608 + 512 > 160 KiB): both passes read K from global memory (ViT-L/14 at 336)
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, HEADS, D = 2, 2, 128
TOKENS = [1, 5, 32, 33, 50, 64, 65, 256, 257, 290, 530, 577]
DTYPES = ["fp16", "bf16"]
TD = {"fp16": torch.float16, "bf16": torch.bfloat16}
U = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}          # half an ulp of a 16-bit value, relative
MANT = {"fp16": 10, "bf16": 7}
MIN_EXP = {"fp16": -14, "bf16": -126}
CANARY = 4096


def _branch(T):
    """The launch rule of csrc/clip_vit.hip (attention_plan + attention_kernel's key split), restated."""
    Tp = (T + 31) // 32 * 32
    att_v, att_k = 64 * (Tp + 4) * 2, Tp * 72 * 2
    assert att_v <= 160 * 1024
    small = 32 < T <= 64
    k_lds = att_v + att_k <= 160 * 1024
    nqb = Tp // 32
    return dict(kernel="small" if small else "main", k_lds=k_lds, nqb=nqb, tail=T % 32 != 0,
                ksplit=(not small) and k_lds and nqb > 8 and nqb % 8 == 1)


EXPECTED_BRANCH = {
    1: dict(kernel="main", k_lds=True, nqb=1, tail=True, ksplit=False),
    5: dict(kernel="main", k_lds=True, nqb=1, tail=True, ksplit=False),
    32: dict(kernel="main", k_lds=True, nqb=1, tail=False, ksplit=False),
    33: dict(kernel="small", k_lds=True, nqb=2, tail=True, ksplit=False),
    50: dict(kernel="small", k_lds=True, nqb=2, tail=True, ksplit=False),
    64: dict(kernel="small", k_lds=True, nqb=2, tail=False, ksplit=False),
    65: dict(kernel="main", k_lds=True, nqb=3, tail=True, ksplit=False),
    256: dict(kernel="main", k_lds=True, nqb=8, tail=False, ksplit=False),
    257: dict(kernel="main", k_lds=True, nqb=9, tail=True, ksplit=True),
    290: dict(kernel="main", k_lds=True, nqb=10, tail=True, ksplit=False),
    530: dict(kernel="main", k_lds=True, nqb=17, tail=True, ksplit=True),
    577: dict(kernel="main", k_lds=False, nqb=19, tail=True, ksplit=False),
}


@pytest.mark.parametrize("T", TOKENS)
def test_every_token_count_takes_its_intended_branch(T):
    assert _branch(T) == EXPECTED_BRANCH[T]
    # the boundaries themselves: K leaves LDS between 576 and 577 tokens, the key split covers exactly 257..288 and 513..544
    assert _branch(576)["k_lds"] and not _branch(577)["k_lds"]
    assert [t for t in range(1, 577) if _branch(t)["ksplit"]] == [*range(257, 289), *range(513, 545)]


def _pack(q, k, v):
    """[B][heads][T][64] each -> the tower's qkv matrix [B*T][3D] = q | k | v, head h in columns 64 h .. 64 h + 63 of its third."""
    T = q.shape[2]
    f = lambda x: x.permute(0, 2, 1, 3).reshape(B * T, D)
    return torch.cat([f(q), f(k), f(v)], 1).contiguous()


def _heads(out, T):
    """[B*T][D] -> [B][heads][T][64]"""
    return out.reshape(B, T, HEADS, 64).permute(0, 2, 1, 3)


def _attention(qkv16, T, dtype):
    """sc_clip_attention on a CPU 16-bit qkv; the output comes back on the CPU.  Every call carries a canary behind row B*T of `out` and
    starts from an output full of NaN: nothing may be written past the end and every row must be written."""
    from shapeclipper_amd import _lib
    lib = _lib.load()
    assert qkv16.dtype == TD[dtype] and qkv16.shape == (B * T, 3 * D)
    buf = torch.full((B * T * D + CANARY,), float("nan"), dtype=TD[dtype], device=DEV)
    buf[B * T * D:] = 7.0
    out = buf[:B * T * D].view(B * T, D)
    q = qkv16.to(DEV)
    rc = lib.sc_clip_attention(_lib.ptr(q), _lib.ptr(out), B, T, D, HEADS, 1 if dtype == "fp16" else 0, _lib.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert (buf[B * T * D:] == 7.0).all(), "sc_clip_attention wrote past row B*T of out"
    res = out.cpu()
    assert torch.isfinite(res.float()).all(), "a row of out was not written (or is not finite)"
    return res


def _bits(x):
    return x.contiguous().view(torch.int16)


# ---- a. one-hot attention: bit-exact -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", TOKENS)
def test_attention_one_hot_is_bit_exact(T, dtype):
    """Key j is 2 code[j] (a random +-1 vector of 64), query i is 2 code[pi(i)]: the logit of the target key is 32, of any other key
    0.5 <code, code'> (|.| <= ~18), so in float64 every query puts less than 2^-13 of its mass off target (asserted) -- the target's
    probability rounds to 1 in 16 bits and what the others add to O stays far below half a 16-bit ulp of v in [1, 2).  The output must
    be v[pi(i)], entries 1 + k/128 (exact in both types), BIT FOR BIT: the key index of every lane of the MFMA C/D layout, the V
    transpose, the masked tail, the round-robin over query blocks and the key-split merge all have to be right for that."""
    assert _branch(T) == EXPECTED_BRANCH[T]
    g = torch.Generator().manual_seed(T)
    code = (torch.randint(0, 2, (B, HEADS, T, 64), generator=g) * 2 - 1).double()
    pi = torch.stack([torch.randperm(T, generator=g) for _ in range(B * HEADS)]).reshape(B, HEADS, T)
    idx = pi[..., None].expand(B, HEADS, T, 64)
    v = 1 + torch.randint(0, 128, (B, HEADS, T, 64), generator=g).double() / 128
    qkv = _pack(2 * code.gather(2, idx), 2 * code, v)
    qkv16 = qkv.to(TD[dtype])
    assert torch.equal(qkv16.double(), qkv)                                    # the inputs are exact in the 16-bit type
    p, _ = ref.attention_probs(qkv, B, T, D, HEADS)
    off = 1 - p.gather(3, pi[..., None]).squeeze(-1)
    assert off.max().item() < 2.0 ** -13, off.max().item()
    want = _pack(v, v, v.gather(2, idx))[:, 2 * D:].to(TD[dtype])              # row b*T + i, head h: v[b][h][pi(i)]
    got = _attention(qkv16, T, dtype)
    wrong = (_bits(got) != _bits(want)).any(1).nonzero().flatten().tolist()
    assert not wrong, "T=%d %s: %d rows differ from v[pi(i)], first rows %s" % (T, dtype, len(wrong), wrong[:8])


# ---- b. uniform attention over exactly T keys -----------------------------------------------------------------------------------------
def _half_ulp16(x, dtype):
    """Half an ulp of the 16-bit type at |x| (float64 tensor), subnormal range included."""
    e = torch.frexp(x.abs().clamp_min(2.0 ** -200))[1] - 1                     # floor(log2 |x|)
    return torch.ldexp(torch.ones_like(x), e.clamp_min(MIN_EXP[dtype]) - MANT[dtype] - 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [2.0, 0.0])
@pytest.mark.parametrize("T", TOKENS)
def test_attention_uniform_over_exactly_T_keys(T, c, dtype):
    """q = -c 1, k = +c 1: c = 2 makes every real logit -32 (a padded key, whose score is 0, would take all the mass); c = 0 makes every
    logit 0.  Either way p = 1 exactly for every real key (the scores are equal and -256 * 0.125 * log2(e) is one exact fp32 product),
    the sums of the small-integer v and of p are exact in fp32, and the output is the mean of v over the T real keys after ONE fp32
    division (O / l, or O * (1 / l): 2^-23 relative) and ONE 16-bit rounding.
    (attention_small_kernel used to round p / l to 16 bits before P V: every key of a flat row then carried the same rounding error,
    and T = 33 / 50 came out at 1.09 / 1.68 (fp16) and 1.45 / 1.28 (bf16) of this budget.  It now divides O by l at the end.)"""
    assert _branch(T) == EXPECTED_BRANCH[T]
    g = torch.Generator().manual_seed(100 + T)
    v = torch.randint(1, 9, (B, HEADS, T, 64), generator=g).double()           # integers 1..8: mean 4.5, never 0
    ones = torch.ones(B, HEADS, T, 64, dtype=torch.float64)
    got = _heads(_attention(_pack(-c * ones, c * ones, v).to(TD[dtype]), T, dtype), T).double()
    mean = v.mean(2, keepdim=True).expand_as(v)
    fp32 = 2.0 ** -23 * mean.abs()
    bar = _half_ulp16(mean.abs() + fp32, dtype) + fp32
    ratio = ((got - mean).abs() / bar).max().item()
    print("uniform attention T=%d c=%g %s: worst error / budget %.3f" % (T, c, dtype, ratio))
    assert ratio <= 1.0, ratio


# ---- c. random attention against float64, derived bound -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("T", TOKENS)
def test_attention_random_vs_float64(T, scale, dtype):
    """q, k ~ scale N(0,1) (scale 4: peaked rows), v ~ N(0,1), rounded to the 16-bit type: exact inputs, so the kernel's own error sources
    are the probabilities rounded to 16 bits (u relative each; fp16 additionally loses p < 2^-14 to an absolute 2^-25 per key), the sum l
    taken from the unrounded p, one 16-bit rounding of the output, fp32 elsewhere.  Per element
        |out - ref| <= 2 [ u (A + |ref|) + T s max|v| ],   A = sum_j p_j |v_j| in float64,
    u = 2^-11, s = 2^-25 (fp16); u = 2^-8, s = 0 (bf16).  The bracket is the first-order bound of those roundings; the factor 2 leaves
    room for the fp32 rounding of scores and exponent, which the test keeps inside it by asserting max |0.125 s| log2(e) 2^-23 <= u / 4
    for its inputs.  A CPU emulation with exactly those rounding points stays <= 0.79 of the bracket (un-doubled)."""
    assert _branch(T) == EXPECTED_BRANCH[T]
    g = torch.Generator().manual_seed(1000 * T + int(scale))
    q, k, v = (torch.randn(B, HEADS, T, 64, generator=g) * s for s in (scale, scale, 1.0))
    qkv16 = _pack(q, k, v).to(TD[dtype])
    qkv = qkv16.double()
    want = ref.attention(qkv, B, T, D, HEADS)
    p, v64 = ref.attention_probs(qkv, B, T, D, HEADS)
    A = (p @ v64.abs()).permute(0, 2, 1, 3).reshape(B * T, D)
    x = qkv.reshape(B, T, 3, HEADS, 64)
    smax = (0.125 * torch.einsum("bihd,bjhd->bhij", x[:, :, 0], x[:, :, 1])).abs().max().item()
    u, s = U[dtype], (2.0 ** -25 if dtype == "fp16" else 0.0)
    assert smax * 1.4427 * 2.0 ** -23 <= u / 4, smax
    bar = 2 * (u * (A + want.abs()) + T * s * v64.abs().max().item())
    got = _attention(qkv16, T, dtype).double()
    ratio = ((got - want).abs() / bar).max().item()
    print("random attention T=%d scale %g %s: worst error / bound %.3f (max |logit| %.1f)" % (T, scale, dtype, ratio, smax))
    assert ratio < 1.0, ratio


# ---- d. refusals, untouched memory -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_refuses_what_the_tower_refuses(dtype):
    """hipErrorInvalidValue (1) for a width that is no multiple of 64, a head dim other than 64 and a V^T tile over 160 KiB (T > 1248);
    nothing is launched: the output keeps its fill.  (Every call of `_attention` above checks the canary behind row B*T.)"""
    from shapeclipper_amd import _lib
    lib = _lib.load()
    fp16 = 1 if dtype == "fp16" else 0
    for b, t, d, h in ((1, 5, 96, 1), (1, 5, 128, 1), (1, 5, 128, 4), (1, 1249, 64, 1), (1, 5, 64, 0), (1, 0, 64, 1)):
        qkv = torch.zeros(b * max(t, 1), 3 * d, dtype=TD[dtype], device=DEV)
        out = torch.full((b * max(t, 1), d), 3.0, dtype=TD[dtype], device=DEV)
        assert lib.sc_clip_attention(_lib.ptr(qkv), _lib.ptr(out), b, t, d, h, fp16, _lib.stream()) == 1, (b, t, d, h)
        torch.cuda.synchronize()
        assert (out == 3.0).all()
    # the largest token count that is accepted runs (V^T = 128 * 1252 bytes, K from global memory)
    T = 1248
    qkv = torch.zeros(T, 192, dtype=TD[dtype], device=DEV)
    qkv[:, 128:] = 1.0
    out = torch.zeros(T, 64, dtype=TD[dtype], device=DEV)
    assert lib.sc_clip_attention(_lib.ptr(qkv), _lib.ptr(out), 1, T, 64, 1, fp16, _lib.stream()) == 0
    torch.cuda.synchronize()
    assert (out == 1.0).all()


# ---- e. LayerNorm against float64 -------------------------------------------------------------------------------------------------------
# The fp32 bar is ref.LN_C * ref.ln_fp32_unit (tests/clip_ref.py: LN_C = 8.44 = 4 x the 2.110 units torch's own float32 LayerNorm reaches on
# exactly these inputs; tests/test_clip_ref_host.py repeats that measurement without a GPU).
LN_C, LN_DIMS, LN_ROWS = ref.LN_C, ref.LN_DIMS, ref.LN_ROWS
OUT16 = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}


def _layernorm(x, stride, g, b, rows, Dm, out_kind, out=None):
    from shapeclipper_amd import _lib
    code, td = OUT16[out_kind]
    if out is None:
        out = torch.full((rows, Dm), float("nan"), dtype=td, device=DEV)
    rc = _lib.load().sc_clip_layernorm(_lib.ptr(x), stride, _lib.ptr(g), _lib.ptr(b), _lib.ptr(out), rows, Dm, ref.LN_EPS, code, _lib.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def _ln_bar(x, g, b, out_kind):
    want = ref.layernorm(x, g, b, ref.LN_EPS)
    bar = LN_C * ref.ln_fp32_unit(x, g, ref.LN_EPS)
    if out_kind != "fp32":
        bar = bar + _half_ulp16(want.abs() + bar, out_kind)
    return want, bar


@pytest.mark.parametrize("out_kind", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("Dm", LN_DIMS)
def test_layernorm_vs_float64(Dm, out_kind):
    """Both code paths of layernorm_kernel (rows in registers: D = 256, 512, 768, 1024 -- 1 to 4 of the 4 register slots; the generic path:
    64, 192, 1088) on 1, 5 and 64 rows (a partial workgroup of four waves, several workgroups), rows D apart and 3 D apart (the ln_post
    use: one row out of T; the floats between are large so that a wrong stride shows), five kinds of rows, every output type.
    Bar per element: LN_C * 2^-24 (max |x_row| / sigma_row + |y^|) |gamma| in fp32, plus half an ulp of the output for the 16-bit types;
    LN_C = 8.44 = 4 x the 2.110 units torch's own float32 LayerNorm reaches on the same inputs (above).  Two runs are bit-identical.
    (The generic path's former one-pass variance ss / D - mean^2 reached 23 x (D = 64), 507 x (192) and 89 x (1088) this bar on the rows
    N(0,1) + 1e3; it is two-pass now.  Measured after that, fp32 output: at most 0.49 of the bar, on constant rows at D = 1088.)"""
    g, b = ref.ln_params(Dm, Dm)
    gd, bd = g.to(DEV), b.to(DEV)
    worst = {}
    for rows in LN_ROWS:
        for kind in ref.LN_INPUTS:
            x = ref.ln_input(kind, rows, Dm, 1000 * Dm + rows)
            want, bar = _ln_bar(x, g, b, out_kind)
            if kind == "constant":
                assert torch.equal(want, b.double().expand(rows, Dm))           # variance 0: the output is beta
            for stride in (Dm, 3 * Dm):
                xs = torch.randn(rows, stride, generator=torch.Generator().manual_seed(stride)) * 50 + 7
                xs[:, :Dm] = x
                xd = xs.to(DEV)
                got = _layernorm(xd, stride, gd, bd, rows, Dm, out_kind)
                again = _layernorm(xd, stride, gd, bd, rows, Dm, out_kind)
                assert torch.equal(got.view(torch.int32 if out_kind == "fp32" else torch.int16),
                                   again.view(torch.int32 if out_kind == "fp32" else torch.int16)), (rows, kind, stride)
                ratio = ((got.cpu().double() - want).abs() / bar).max().item()
                worst[kind] = max(worst.get(kind, 0.0), ratio)
                assert ratio <= 1.0, (rows, kind, stride, ratio)
    print("LayerNorm D=%d -> %s: worst error / bar %s" % (Dm, out_kind, ", ".join("%s %.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("Dm", LN_DIMS)
def test_layernorm_fp32_in_place(Dm):
    """ln_pre writes the fp32 residual stream over its own input (out == x, stride == D): the same values as out of place, bit for bit."""
    g, b = ref.ln_params(Dm, Dm)
    gd, bd = g.to(DEV), b.to(DEV)
    for rows in LN_ROWS:
        for kind in ref.LN_INPUTS:
            x = ref.ln_input(kind, rows, Dm, 1000 * Dm + rows)
            want, bar = _ln_bar(x, g, b, "fp32")
            xd = x.to(DEV)
            apart = _layernorm(xd, Dm, gd, bd, rows, Dm, "fp32")
            inplace = _layernorm(xd, Dm, gd, bd, rows, Dm, "fp32", out=xd)
            assert inplace.data_ptr() == xd.data_ptr() and torch.equal(inplace.view(torch.int32), apart.view(torch.int32)), (rows, kind)
            assert ((inplace.cpu().double() - want).abs() <= bar).all(), (rows, kind)


def test_layernorm_refuses_bad_arguments():
    from shapeclipper_amd import _lib
    x = torch.zeros(4, 64, device=DEV)
    for stride, rows, Dm, code in ((32, 4, 64, 0), (64, 0, 64, 0), (64, 4, 0, 0), (64, 4, 64, 3), (64, 4, 64, -1)):
        assert _lib.load().sc_clip_layernorm(_lib.ptr(x), stride, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), rows, Dm, 1e-5, code, _lib.stream()) == 1


# ---- f. zero-layer tower: patch gather, patch GEMM, class / position embedding, ln_pre, ln_post, projection ------------------------------
def _align256(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,W,patch", [(64, 96, 32), (56, 28, 14)])      # a 2 x 3 grid (T = 7, 16-byte gather path); 4 x 2, K = 588 padded to 640
def test_zero_layer_tower_places_every_pixel(H, W, patch, dtype):
    """sc_clip_vit_forward* with layers = 0 on NON-square images and structured inputs: the image is an integer ramp over (channel, row,
    column) (wrapped so that it is exact in the 16-bit type), filter d of the patch embedding selects ONE pixel k_d of the patch
    (k_d = 37 d + 5 mod 3 P^2 runs over channels, rows and columns), so token 1 + i of the residual stream holds, in coordinate d, exactly
    the pixel (channel, row, column)(k_d) of patch i plus a position embedding that is distinct per token.  A transposed patch grid or a
    wrong (channel, row, column) order inside a patch moves pixels between coordinates.
    Checked: the embedding (class token -> ln_pre -> ln_post -> projection) against clip_ref.tower at the tower's bars; the residual
    stream after ln_pre (read from the workspace: a_patch, patch_out, x in the documented carve order) against float64 at the LayerNorm
    bar; and, gamma = 1, beta = 0, the arg-max token of every coordinate and the arg-max coordinate of every token, where the reference's
    own margin is asserted to be far above the bar."""
    from shapeclipper_amd import _lib
    lib = _lib.load()
    C, Dm, proj, mlp = 3, D, 64, 256
    gh, gw = H // patch, W // patch
    np_, K = gh * gw, C * patch * patch
    T, Kp = np_ + 1, (K + 63) // 64 * 64
    wrap = 2048 if dtype == "fp16" else 256
    ramp = (torch.arange(C)[:, None, None] * H * W + torch.arange(H)[None, :, None] * W + torch.arange(W)[None, None, :])
    image = torch.stack([((ramp + 17 * b) % wrap - wrap // 2).float() / 16 for b in range(B)])
    assert torch.equal(image.to(TD[dtype]).float(), image)
    kd = (37 * torch.arange(Dm) + 5) % K
    w_patch = torch.zeros(Dm, K)
    w_patch[torch.arange(Dm), kd] = 1.0
    g = torch.Generator().manual_seed(H)
    cls = torch.randn(Dm, generator=g)
    pos = 0.5 * torch.arange(T, dtype=torch.float32)[:, None] + torch.randn(T, Dm, generator=g)
    w_proj = (torch.randn(proj, Dm, generator=g) / Dm ** 0.5).to(TD[dtype])
    post_g, post_b = ref.ln_params(Dm, 3)
    vm = "vision_model."
    sd = {vm + "embeddings.patch_embedding.weight": w_patch.reshape(Dm, C, patch, patch), vm + "embeddings.class_embedding": cls,
          vm + "embeddings.position_embedding.weight": pos, vm + "pre_layrnorm.weight": torch.ones(Dm), vm + "pre_layrnorm.bias": torch.zeros(Dm),
          vm + "post_layernorm.weight": post_g, vm + "post_layernorm.bias": post_b, "visual_projection.weight": w_proj.float()}
    want = ref.tower(image, sd, patch, HEADS, 0)
    x_want = ref.layernorm(ref.embed(image, w_patch, cls, pos, patch), torch.ones(Dm), torch.zeros(Dm), 1e-5)

    w16 = torch.cat([torch.nn.functional.pad(w_patch, (0, Kp - K)).reshape(-1).to(TD[dtype]), w_proj.reshape(-1)]).to(DEV)
    w32 = torch.cat([cls, pos.reshape(-1), torch.ones(Dm), torch.zeros(Dm), post_g, post_b]).float().to(DEV)
    nbytes = lib.sc_clip_vit_workspace_bytes(B, C, H, W, patch, Dm, mlp)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.full((B, proj), float("nan"), device=DEV)
    fn = lib.sc_clip_vit_forward_f16 if dtype == "fp16" else lib.sc_clip_vit_forward
    image_d = image.to(DEV)
    rc = fn(_lib.ptr(image_d), B, C, H, W, patch, Dm, mlp, 0, HEADS, proj, _lib.ptr(w16), _lib.ptr(w32), 1e-5, _lib.ptr(out), _lib.ptr(ws),
            nbytes, _lib.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    # the embedding at the tower's bars (tests/test_gpu_clip.py)
    got = out.cpu().double()
    cos = torch.nn.functional.cosine_similarity(got, want, dim=-1).min().item()
    err = (got - want).abs().max().item() / want.abs().max().item()
    print("zero-layer tower %dx%d patch %d %s: min cosine %.7f, max abs error %.3f %% of max |ref|" % (H, W, patch, dtype, cos, 100 * err))
    cos_bar, err_bar = {"fp16": (0.99999, 0.004), "bf16": (0.9999, 0.025)}[dtype]
    assert torch.isfinite(got).all() and cos > cos_bar and err < err_bar
    # the residual stream after ln_pre
    off = _align256(B * np_ * Kp * 2) + _align256(B * np_ * Dm * 4)
    x_got = ws[off:off + B * T * Dm * 4].view(torch.float32).reshape(B, T, Dm).cpu().double()
    # the kernel normalises fl32(patch + pos): one fp32 rounding of every entry (<= 2^-24 max |x_row|) moves a normalised value by at most
    # twice that over sigma_row (its own entry and the mean), on top of the LayerNorm bar
    x_pre = ref.embed(image, w_patch, cls, pos, patch)
    sigma = torch.sqrt(x_pre.var(-1, unbiased=False, keepdim=True) + 1e-5)
    bar = LN_C * ref.ln_fp32_unit(x_pre, torch.ones(Dm), 1e-5) + 2.0 ** -23 * x_pre.abs().amax(-1, keepdim=True) / sigma
    ratio = ((x_got - x_want).abs() / bar).max().item()
    print("  residual stream after ln_pre: worst error / bar %.3f" % ratio)
    assert ratio <= 1.0, ratio
    for dim in (1, 2):                                                     # arg-max token per coordinate, arg-max coordinate per token
        top = x_want.topk(2, dim=dim).values
        clear = (top.select(dim, 0) - top.select(dim, 1)) > 100 * bar.max()        # the reference's own margin is far above the bar
        assert clear.float().mean().item() > 0.9
        assert torch.equal(x_got.argmax(dim)[clear], x_want.argmax(dim)[clear]), dim
