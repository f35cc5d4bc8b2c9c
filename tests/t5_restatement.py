"""TEST INFRASTRUCTURE ONLY -- a plain-torch restatement of the T5 v1.1 encoder (transformers' T5EncoderModel with
feed_forward_proj="gated-gelu") as functions over a state dict with the Hugging Face keys.  It runs in the dtype of the state dict
(fp32: the truth of the parity tests; bf16: their comparator, rounding where the Hugging Face modules round) on any device.
Pinned to transformers' own output by tests/golden/t5_small.npz (tools/make_golden_t5.py) and, where transformers imports, to the
live model (tests/test_t5_host.py).  Never imported by the product path."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

# the small test geometry: distances pass max_distance at L = 192
SMALL = dict(vocab_size=128, d_model=256, d_kv=64, d_ff=512, num_layers=2, num_heads=4, relative_attention_num_buckets=32,
             relative_attention_max_distance=128, layer_norm_epsilon=1e-6)
# one layer at the width of T5-v1.1-XXL (the GEMM shapes of the shipped encoder), a small vocabulary
XXL_LAYER = dict(vocab_size=256, d_model=4096, d_kv=64, d_ff=10240, num_layers=1, num_heads=64, relative_attention_num_buckets=32,
                 relative_attention_max_distance=128, layer_norm_epsilon=1e-6)


def param_shapes(cfg: dict) -> dict:
    """state-dict key -> shape, in transformers' order"""
    D, inner, F_ = cfg["d_model"], cfg["num_heads"] * cfg["d_kv"], cfg["d_ff"]
    s = {"shared.weight": (cfg["vocab_size"], D), "encoder.embed_tokens.weight": (cfg["vocab_size"], D)}
    for n in range(cfg["num_layers"]):
        a, f = f"encoder.block.{n}.layer.0.", f"encoder.block.{n}.layer.1."
        for w in "qkv":
            s[a + f"SelfAttention.{w}.weight"] = (inner, D)
        s[a + "SelfAttention.o.weight"] = (D, inner)
        if n == 0:
            s[a + "SelfAttention.relative_attention_bias.weight"] = (cfg["relative_attention_num_buckets"], cfg["num_heads"])
        s[a + "layer_norm.weight"] = (D,)
        s[f + "DenseReluDense.wi_0.weight"] = (F_, D)
        s[f + "DenseReluDense.wi_1.weight"] = (F_, D)
        s[f + "DenseReluDense.wo.weight"] = (D, F_)
        s[f + "layer_norm.weight"] = (D,)
    s["encoder.final_layer_norm.weight"] = (D,)
    return s


def make_state_dict(cfg: dict, seed: int = 0, device="cpu") -> dict:
    """seeded, bf16-representable fp32 weights: Linears N(0, 1/fan_in), the embedding N(0, 1), norm weights 1 + 0.1 N, and a
    relative-attention bias of N(0, 2^2) so that the bias decides which keys a head attends"""
    g = torch.Generator(device=device).manual_seed(1000003 * seed + 29)
    sd = {}
    for name, shape in param_shapes(cfg).items():
        if name == "encoder.embed_tokens.weight":
            sd[name] = sd["shared.weight"]
            continue
        r = torch.randn(shape, generator=g, device=device)
        if name.endswith("layer_norm.weight"):
            r = 1.0 + 0.1 * r
        elif name.endswith("relative_attention_bias.weight"):
            r = 2.0 * r
        elif name != "shared.weight":
            r = r * shape[1] ** -0.5
        sd[name] = r.bfloat16().float()
    return sd


def relative_position_bucket(relative_position, num_buckets=32, max_distance=128):
    """T5Attention._relative_position_bucket with bidirectional=True"""
    num_buckets //= 2
    relative_buckets = (relative_position > 0).to(torch.long) * num_buckets
    relative_position = torch.abs(relative_position)
    max_exact = num_buckets // 2
    is_small = relative_position < max_exact
    if_large = max_exact + (torch.log(relative_position.float() / max_exact) / math.log(max_distance / max_exact)
                            * (num_buckets - max_exact)).to(torch.long)
    if_large = torch.min(if_large, torch.full_like(if_large, num_buckets - 1))
    return relative_buckets + torch.where(is_small, relative_position, if_large)


def compute_bias(sd: dict, cfg: dict, L: int) -> torch.Tensor:
    """T5Attention.compute_bias(L, L) without its leading 1: [H, L, L] in the dtype of the embedding"""
    w = sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
    pos = torch.arange(L, device=w.device)
    buckets = relative_position_bucket(pos[None, :] - pos[:, None], cfg["relative_attention_num_buckets"],
                                       cfg["relative_attention_max_distance"])
    return w[buckets].permute(2, 0, 1)


def toeplitz_table(full: torch.Tensor) -> torch.Tensor:
    """[H, L, L] with entries that depend on j - i alone -> [H, 2 L - 1] indexed by (j - i) + L - 1 (asserts the premise)"""
    H, L, _ = full.shape
    table = torch.cat([full[:, :, 0].flip(1), full[:, 0, 1:]], 1)
    idx = torch.arange(L)[None, :] - torch.arange(L)[:, None] + L - 1
    assert torch.equal(table[:, idx], full), "the bias is not a function of j - i"
    return table


def layer_norm(x, w, eps):
    """T5LayerNorm: no mean subtraction, f32 statistics; a half-precision weight rounds the normalised value first"""
    var = x.to(torch.float32).pow(2).mean(-1, keepdim=True)
    x = x * torch.rsqrt(var + eps)
    if w.dtype in (torch.float16, torch.bfloat16):
        x = x.to(w.dtype)
    return w * x


def attention(q, k, v, bias, scale=1.0):
    """q, k, v [B, L, H, hd]; bias [H, L, L] | None -> [B, L, H, hd]: softmax in f32, cast back (T5Attention.forward)"""
    scores = torch.matmul(q.transpose(1, 2), k.transpose(1, 2).transpose(2, 3))
    if scale != 1.0:
        scores = scores * scale
    if bias is not None:
        scores = scores + bias
    w = F.softmax(scores.float(), dim=-1).type_as(scores)
    return torch.matmul(w, v.transpose(1, 2)).transpose(1, 2)


def encode(sd: dict, cfg: dict, input_ids: torch.Tensor) -> torch.Tensor:
    """T5EncoderModel(input_ids, attention_mask=None).last_hidden_state in eval mode"""
    B, L = input_ids.shape
    H, hd, eps = cfg["num_heads"], cfg["d_kv"], cfg["layer_norm_epsilon"]
    x = sd["shared.weight"][input_ids]
    bias = compute_bias(sd, cfg, L)
    for n in range(cfg["num_layers"]):
        a, f = f"encoder.block.{n}.layer.0.", f"encoder.block.{n}.layer.1."
        h = layer_norm(x, sd[a + "layer_norm.weight"], eps)
        q, k, v = ((h @ sd[a + f"SelfAttention.{w}.weight"].T).view(B, L, H, hd) for w in "qkv")
        ctx = attention(q, k, v, bias).reshape(B, L, H * hd)
        x = x + ctx @ sd[a + "SelfAttention.o.weight"].T
        h = layer_norm(x, sd[f + "layer_norm.weight"], eps)
        g = F.gelu(h @ sd[f + "DenseReluDense.wi_0.weight"].T, approximate="tanh") * (h @ sd[f + "DenseReluDense.wi_1.weight"].T)
        x = x + g @ sd[f + "DenseReluDense.wo.weight"].T
    return layer_norm(x, sd["encoder.final_layer_norm.weight"], eps)
