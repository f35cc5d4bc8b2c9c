"""TEST INFRASTRUCTURE ONLY -- a plain-torch restatement of the CLIP text encoder (transformers' CLIPTextModel with
hidden_act="quick_gelu") as functions over a state dict with the Hugging Face keys (transformers 5: no `text_model.` prefix).  It
runs in the dtype of the state dict (fp32: the truth of the parity tests; bf16: their comparator, rounding after every module as
the Hugging Face modules do) on any device.  Pinned to transformers' own output by tests/golden/clip_small.npz
(tools/make_golden_clip.py) and, where transformers imports, to the live model (tests/test_clip_host.py).  Never imported by the
product path."""
from __future__ import annotations

import torch
import torch.nn.functional as F

# the small test geometry: 77 positions = one full 64-key tile and a diagonal tile with a tail
SMALL = dict(vocab_size=512, hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2,
             max_position_embeddings=77, layer_norm_eps=1e-5, eos_token_id=2)
# one layer at the width of CLIP ViT-L/14's text tower (the GEMM shapes of the shipped encoder), a small vocabulary
L_LAYER = dict(vocab_size=512, hidden_size=768, intermediate_size=3072, num_hidden_layers=1, num_attention_heads=12,
               max_position_embeddings=77, layer_norm_eps=1e-5, eos_token_id=2)


def param_shapes(cfg: dict) -> dict:
    """state-dict key -> shape, in transformers' order"""
    D, F_ = cfg["hidden_size"], cfg["intermediate_size"]
    s = {"embeddings.token_embedding.weight": (cfg["vocab_size"], D),
         "embeddings.position_embedding.weight": (cfg["max_position_embeddings"], D)}
    for n in range(cfg["num_hidden_layers"]):
        ly = f"encoder.layers.{n}."
        for w in ("k_proj", "v_proj", "q_proj", "out_proj"):
            s[ly + f"self_attn.{w}.weight"] = (D, D)
            s[ly + f"self_attn.{w}.bias"] = (D,)
        s[ly + "layer_norm1.weight"] = s[ly + "layer_norm1.bias"] = (D,)
        s[ly + "mlp.fc1.weight"], s[ly + "mlp.fc1.bias"] = (F_, D), (F_,)
        s[ly + "mlp.fc2.weight"], s[ly + "mlp.fc2.bias"] = (D, F_), (D,)
        s[ly + "layer_norm2.weight"] = s[ly + "layer_norm2.bias"] = (D,)
    s["final_layer_norm.weight"] = s["final_layer_norm.bias"] = (D,)
    return s


def make_state_dict(cfg: dict, seed: int = 0, device="cpu") -> dict:
    """seeded, bf16-representable fp32 weights: Linear weights N(0, 1/fan_in) -- q and k twice that, so that the scores spread over
    a few units and the softmax is far from uniform --, the token table N(0, 1), the position table N(0, 0.5^2), norm weights
    1 + 0.1 N, every bias 0.1 N"""
    g = torch.Generator(device=device).manual_seed(1000003 * seed + 41)
    sd = {}
    for name, shape in param_shapes(cfg).items():
        r = torch.randn(shape, generator=g, device=device)
        if name.endswith(".bias"):
            r = 0.1 * r
        elif "layer_norm" in name:
            r = 1.0 + 0.1 * r
        elif name == "embeddings.position_embedding.weight":
            r = 0.5 * r
        elif name != "embeddings.token_embedding.weight":
            r = r * shape[1] ** -0.5 * (2.0 if ("q_proj" in name or "k_proj" in name) else 1.0)
        sd[name] = r.bfloat16().float()
    return sd


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def attention(q, k, v, scale):
    """q, k, v [B, L, H, hd] -> [B, L, H, hd]: causal (key j visible to query i when j <= i), softmax in f32, cast back"""
    L = q.shape[1]
    scores = torch.matmul(q.transpose(1, 2), k.transpose(1, 2).transpose(2, 3)) * scale
    above = torch.ones(L, L, dtype=torch.bool, device=q.device).triu(1)
    scores = scores.masked_fill(above, float("-inf"))
    w = F.softmax(scores.float(), dim=-1).type_as(scores)
    return torch.matmul(w, v.transpose(1, 2)).transpose(1, 2)


def pool(last_hidden_state, input_ids, eos_token_id):
    """the row transformers pools: eos_token_id 2 (the configurations of the published checkpoints) takes the LARGEST id of a row,
    any other value the first position equal to it"""
    if eos_token_id == 2:
        at = input_ids.argmax(-1)
    else:
        at = (input_ids == eos_token_id).int().argmax(-1)
    return last_hidden_state[torch.arange(input_ids.shape[0], device=last_hidden_state.device), at]


def encode(sd: dict, cfg: dict, input_ids: torch.Tensor):
    """CLIPTextModel(input_ids, attention_mask=None) in eval mode -> (last_hidden_state, pooler_output)"""
    B, L = input_ids.shape
    D, H, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["layer_norm_eps"]
    hd = D // H
    lin = lambda x, name: F.linear(x, sd[name + ".weight"], sd[name + ".bias"])                      # noqa: E731
    ln = lambda x, name: F.layer_norm(x, (D,), sd[name + ".weight"], sd[name + ".bias"], eps)          # noqa: E731
    x = sd["embeddings.token_embedding.weight"][input_ids] + sd["embeddings.position_embedding.weight"][:L]
    for n in range(cfg["num_hidden_layers"]):
        ly = f"encoder.layers.{n}."
        h = ln(x, ly + "layer_norm1")
        q, k, v = (lin(h, ly + f"self_attn.{w}_proj").view(B, L, H, hd) for w in "qkv")
        x = x + lin(attention(q, k, v, hd ** -0.5).reshape(B, L, D), ly + "self_attn.out_proj")
        h = ln(x, ly + "layer_norm2")
        x = x + lin(quick_gelu(lin(h, ly + "mlp.fc1")), ly + "mlp.fc2")
    y = ln(x, "final_layer_norm")
    return y, pool(y, input_ids, cfg["eos_token_id"])
