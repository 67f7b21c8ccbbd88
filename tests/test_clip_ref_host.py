"""tests/clip_ref.py (the float64 restatement of the CLIP tower's stages the GPU stage tests compare against) on the CPU: composed into
`tower` it must reproduce BOTH architecture oracles evaluated in float64 on the same weights -- oracle/clip_openai_ref.py (the original
package's modules, torch's nn.MultiheadAttention) and transformers.CLIPVisionModelWithProjection -- to 1e-10 of the embedding's scale.
At that bar every stage function is pinned: a wrong patch order, head split, softmax scale, variance or QuickGELU constant is an error
of order 1."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as ref  # noqa: E402

from oracle import clip_openai_ref as O  # noqa: E402
from shapeclipper_amd.model.clip_vit import ClipVisionTower  # noqa: E402

RES, PATCH, WIDTH, PROJ = 48, 8, 128, 64           # 6 x 6 patches + class token = 37 tokens, 2 heads


@pytest.mark.parametrize("layers", [0, 2])
def test_tower_restatement_matches_both_architecture_oracles_in_float64(layers):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    oa, sd = O.seeded(RES, PATCH, WIDTH, layers, PROJ, seed=17 + layers)
    oa = oa.double()
    cfg = dict(image_size=RES, patch=PATCH, width=WIDTH, layers=layers, heads=WIDTH // 64, mlp=4 * WIDTH, proj=PROJ)
    tsd = ClipVisionTower.from_openai_state_dict(sd, **cfg).state_dict()          # the tower's (transformers') names, fp32 values
    hf = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_size=WIDTH, intermediate_size=4 * WIDTH, num_hidden_layers=layers,
                                                        num_attention_heads=WIDTH // 64, patch_size=PATCH, image_size=RES,
                                                        projection_dim=PROJ, hidden_act="quick_gelu")).eval()
    missing, unexpected = hf.load_state_dict(tsd, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    hf = hf.double()
    x = torch.randn(3, 3, RES, RES, generator=torch.Generator().manual_seed(1)).double()
    with torch.no_grad():
        a, b = oa.encode_image(x), hf(pixel_values=x).image_embeds
    got = ref.tower(x, tsd, PATCH, WIDTH // 64, layers)
    assert got.dtype == torch.float64 and got.shape == (3, PROJ)
    scale = a.abs().max().item()
    print("clip_ref.tower, %d layers: |vs openai modules| %.2e, |vs transformers| %.2e of scale %.3f"
          % (layers, (got - a).abs().max().item() / scale, (got - b).abs().max().item() / scale, scale))
    assert (got - a).abs().max().item() <= 1e-10 * scale
    assert (got - b).abs().max().item() <= 1e-10 * scale


def test_stage_functions_on_hand_computable_inputs():
    """The pieces on inputs whose answer is known without a formula to trust."""
    # attention: two tokens, one head; q . k = 0 everywhere -> uniform -> the mean of v
    qkv = torch.zeros(2, 192, dtype=torch.float64)
    qkv[0, 128:], qkv[1, 128:] = 1.0, 3.0
    assert torch.equal(ref.attention(qkv, 1, 2, 64, 1), torch.full((2, 64), 2.0, dtype=torch.float64))
    # two images are independent, and the second head reads columns 64..127 of each third
    qkv = torch.randn(6, 384, generator=torch.Generator().manual_seed(0)).double()
    full = ref.attention(qkv, 2, 3, 128, 2)
    one = ref.attention(qkv[3:, [*range(64, 128), *range(192, 256), *range(320, 384)]], 1, 3, 64, 1)
    assert torch.allclose(full[3:, 64:], one, rtol=0, atol=1e-15)
    # layernorm: a row (1, 3) has mean 2 and variance 1
    y = ref.layernorm(torch.tensor([[1.0, 3.0]]), torch.tensor([2.0, 2.0]), torch.tensor([0.5, 0.5]), 0.0)
    assert torch.equal(y, torch.tensor([[-1.5, 2.5]], dtype=torch.float64))
    # patches: a 2 x 3 grid of 2 x 2 patches of an image whose value encodes (channel, row, column)
    img = (torch.arange(2)[:, None, None] * 100 + torch.arange(4)[None, :, None] * 10 + torch.arange(6)[None, None, :])[None].double()
    p = ref.patches(img, 2)
    assert p.shape == (1, 6, 8)
    assert p[0, 0].tolist() == [0, 1, 10, 11, 100, 101, 110, 111]                  # (channel, row, column) inside a patch
    assert p[0, 1, 0].item() == 2 and p[0, 3, 0].item() == 20                       # patch 1 is to the RIGHT, patch 3 starts the next row
    # embed: the class token in front, positions added per token
    e = ref.embed(img, torch.eye(8).reshape(8, 2, 2, 2), torch.full((8,), -1.0), torch.arange(7.0)[:, None].expand(7, 8), 2)
    assert e.shape == (1, 7, 8) and e[0, 0].tolist() == [-1.0] * 8 and e[0, 2].tolist() == [v + 2 for v in p[0, 1].tolist()]


def test_layernorm_bar_constant_is_four_times_torchs_float32_error():
    """LN_C (the fp32 bar of tests/test_gpu_clip_stages.py) is 4 x what a plain two-pass float32 LayerNorm reaches on the same inputs, not a
    figure read off the HIP kernel.  torch's CPU kernel may order its sums differently on another vector width: the check is a band."""
    worst = ref.ln_torch_fp32_worst()
    print("torch float32 LayerNorm vs float64: worst %.3f units of 2^-24 (max|x|/sigma + |y^|) |gamma|; LN_C = %.2f" % (worst, ref.LN_C))
    assert ref.LN_C / 6 <= worst <= ref.LN_C / 3
