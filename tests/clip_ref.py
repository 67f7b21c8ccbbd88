"""TEST INFRASTRUCTURE ONLY.  The stages of the CLIP ViT image tower (csrc/clip_vit.hip) restated in plain float64 torch, one function
per kernel family, so that a HIP kernel can be compared with the operation it implements and not only through the whole tower:

    attention   softmax(0.125 q k^T) v per image and head on a packed [B*T][3D] = q | k | v matrix (head dim 64 -> scale 1/8)
    layernorm   (x - mean) / sqrt(var + eps) * gamma + beta over the last axis, biased variance
    embed       non-overlapping patches in (row, column) order, each flattened (channel, row, column) -> @ w_patch^T, class token in
                front, position embedding added
    tower       embed -> ln_pre -> layers x {x += out_proj(attention(qkv(ln_1 x))); x += fc2(quick_gelu(fc1(ln_2 x)))} ->
                ln_post(x[:, 0]) @ proj^T, for any layer count including 0

tests/test_clip_ref_host.py ties `tower` to oracle/clip_openai_ref.py and to transformers' model in float64 (1e-10 of scale), which pins
these functions to the architecture before the GPU tests use them.  Weights come as a state dict in the tower's own (transformers') names.
"""
import torch

F64 = torch.float64


def attention_probs(qkv, B, T, D, heads):
    """p [B][heads][T query][T key] float64 and v [B][heads][T][64] of a packed qkv [B*T][3D]."""
    x = qkv.to(F64).reshape(B, T, 3, heads, D // heads)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))                 # [B][heads][T][64]
    s = 0.125 * (q @ k.transpose(-1, -2))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    return p / p.sum(-1, keepdim=True), v


def attention(qkv, B, T, D, heads):
    """[B*T][3D] -> [B*T][D] float64."""
    assert D // heads == 64 and D % 64 == 0
    p, v = attention_probs(qkv, B, T, D, heads)
    return (p @ v).permute(0, 2, 1, 3).reshape(B * T, D)


def layernorm(x, g, b, eps):
    x = x.to(F64)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * g.to(F64) + b.to(F64)


LN_EPS = 1e-5
LN_INPUTS = ("n01", "offset1e3", "massive300", "constant", "tiny1e-3")


def ln_input(kind, rows, D, seed):
    """fp32 [rows][D] test rows of the LayerNorm stage tests: N(0,1); N(0,1) + 1e3 (a mean large against the spread: the one-pass variance
    cancels); N(0,1) with one channel at 300 (the "massive activation" rows of real CLIP checkpoints); constant rows (variance 0: the
    output is beta); rows of magnitude 1e-3, where the variance is of the order of eps."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g)
    if kind == "offset1e3":
        x = x + 1e3
    elif kind == "massive300":
        x[torch.arange(rows), torch.randint(0, D, (rows,), generator=g)] = 300.0
    elif kind == "constant":
        x = (0.37 + 2.9 * torch.arange(rows, dtype=torch.float32))[:, None].expand(rows, D).contiguous()
    elif kind == "tiny1e-3":
        x = 1e-3 * x
    else:
        assert kind == "n01", kind
    return x.float()


def ln_params(D, seed):
    g = torch.Generator().manual_seed(seed)
    return (1 + 0.1 * torch.randn(D, generator=g)).float(), (0.1 * torch.randn(D, generator=g)).float()


def ln_fp32_unit(x, g, eps):
    """2^-24 (max |x_row| / sigma_row + |y^|) |gamma| per element, float64: the fp32 bar of the LayerNorm tests is c times this.  The first
    term is what one fp32 rounding of the mean (of the size of the row's largest entry) does to the normalised value, the second one
    rounding of the normalised value itself."""
    x = x.to(F64)
    mean = x.mean(-1, keepdim=True)
    sigma = torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    return 2.0 ** -24 * (x.abs().amax(-1, keepdim=True) / sigma + ((x - mean) / sigma).abs()) * g.to(F64).abs()


# c of the fp32 LayerNorm bar c * ln_fp32_unit.  Not taken from the kernel: torch's own two-pass float32 LayerNorm on the CPU
# (torch.nn.functional.layer_norm) against float64 on exactly the inputs of the stage tests (every D, row count and input kind below)
# reaches at most 2.110 units (n01 2.01, offset1e3 1.93, massive300 2.11, constant 0, tiny1e-3 1.58); c = 4 x 2.110.
LN_C = 8.44
LN_DIMS = [64, 192, 256, 512, 768, 1024, 1088]
LN_ROWS = [1, 5, 64]


def ln_torch_fp32_worst():
    """The measurement behind LN_C: worst error of torch's float32 LayerNorm on the CPU in units of ln_fp32_unit."""
    worst = 0.0
    for D in LN_DIMS:
        g, b = ln_params(D, D)
        for rows in LN_ROWS:
            for kind in LN_INPUTS:
                x = ln_input(kind, rows, D, 1000 * D + rows)
                y = torch.nn.functional.layer_norm(x, (D,), g, b, LN_EPS).to(F64)
                worst = max(worst, ((y - layernorm(x, g, b, LN_EPS)).abs() / ln_fp32_unit(x, g, LN_EPS)).max().item())
    return worst


def patches(image, patch):
    """[B][C][H][W] -> [B][(H/patch)*(W/patch)][C*patch*patch] float64: patch (py, px) is row py * (W/patch) + px, its pixels flattened
    in (channel, row, column) order -- the layout of a stride-`patch` convolution's weight [D][C][patch][patch]."""
    B, C, H, W = image.shape
    gh, gw = H // patch, W // patch
    x = image.to(F64)[:, :, :gh * patch, :gw * patch].reshape(B, C, gh, patch, gw, patch)
    return x.permute(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, C * patch * patch)


def embed(image, w_patch, cls, pos, patch):
    """tokens [B][T][D] float64, T = patches + 1: [class; patches @ w_patch^T] + pos."""
    D = w_patch.shape[0]
    tok = patches(image, patch) @ w_patch.to(F64).reshape(D, -1).t()
    x = torch.cat([cls.to(F64).expand(tok.shape[0], 1, D), tok], 1)
    return x + pos.to(F64)


def tower(image, sd, patch, heads, layers, eps=1e-5):
    """image [B][C][H][W] -> embedding [B][proj] float64 (not L2-normalised)."""
    g = lambda n: sd[n].to(F64)
    vm = "vision_model."
    x = embed(image, g(vm + "embeddings.patch_embedding.weight"), g(vm + "embeddings.class_embedding"),
              g(vm + "embeddings.position_embedding.weight"), patch)
    B, T, D = x.shape
    x = layernorm(x, g(vm + "pre_layrnorm.weight"), g(vm + "pre_layrnorm.bias"), eps)
    for l in range(layers):
        pre = vm + "encoder.layers.%d." % l
        lin = lambda y, n: y @ g(pre + n + ".weight").t() + g(pre + n + ".bias")
        y = layernorm(x, g(pre + "layer_norm1.weight"), g(pre + "layer_norm1.bias"), eps)
        qkv = torch.cat([lin(y, "self_attn.%s" % n) for n in ("q_proj", "k_proj", "v_proj")], -1)
        x = x + lin(attention(qkv.reshape(B * T, 3 * D), B, T, D, heads).reshape(B, T, D), "self_attn.out_proj")
        h = lin(layernorm(x, g(pre + "layer_norm2.weight"), g(pre + "layer_norm2.bias"), eps), "mlp.fc1")
        x = x + lin(h * torch.sigmoid(1.702 * h), "mlp.fc2")
    return layernorm(x[:, 0], g(vm + "post_layernorm.weight"), g(vm + "post_layernorm.bias"), eps) @ g("visual_projection.weight").t()
