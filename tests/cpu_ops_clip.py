"""TEST INFRASTRUCTURE ONLY -- tests/cpu_ops_t5.py (the CPU emulation of the kernel table) plus the three entry points of the CLIP
text encoder: osk_layernorm_affine_bf16 (csrc/layernorm.hip), osk_attention_causal_bf16 (csrc/attention_relbias.hip) and
osk_gemm_quickgelu_bf16 (csrc/gemm_bf16.hip), with the Python call signatures of open_sora_amd/_C.py.  Never imported by the product
path.  The `*_ref` functions are the formulas of include/osk.h in a chosen dtype before the output rounding and run on any device;
the table functions do the math in fp32 on the bf16-stored operands, rounded once."""
from __future__ import annotations

import torch

from tests.cpu_ops_t5 import *  # noqa: F401,F403  (the rest of the kernel table)
from tests.cpu_ops_t5 import _abi_check, _al


def layernorm_affine_ref(x, weight, bias, eps=1e-5, dtype=torch.float32):
    """(x - mean) * rsqrt(var + eps) * weight + bias, biased variance of the centred values; every operation in `dtype`"""
    xs = x.to(dtype)
    c = xs - xs.mean(-1, keepdim=True)
    return c * torch.rsqrt(c.square().mean(-1, keepdim=True) + eps) * weight.to(dtype) + bias.to(dtype)


def attention_causal_ref(q, k, v, H, hd, scale, dtype=torch.float32):
    """out[b, i, h] = sum_{j <= i} softmax_j(scale q_i . k_j) v_j;  q, k, v [B, L, H * hd].  Every operation in `dtype` (bf16: a
    reference-precision evaluation that materialises and rounds the scores)."""
    B, L, _ = q.shape
    qh, kh, vh = (t.to(dtype).reshape(B, L, H, hd).transpose(1, 2) for t in (q, k, v))
    s = (qh @ kh.transpose(2, 3)) * scale
    s = s.masked_fill(torch.ones(L, L, dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, L, H * hd)


def quick_gelu_ref(v):
    return v * torch.sigmoid(1.702 * v)


def gemm_quickgelu_ref(a, w, bias, dtype=torch.float32):
    y = a.to(dtype) @ w.to(dtype).T
    if bias is not None:
        y = y + bias.to(dtype)
    return quick_gelu_ref(y)


# ---- the kernel table entries (signatures of open_sora_amd/_C.py)
def layernorm_affine(x, weight, bias, out, eps=1e-5):
    C = x.shape[-1]
    if C % 8 or C > 4096:
        raise RuntimeError("osk_layernorm_affine_bf16 failed: status -2 (invalid argument / unsupported shape)")
    _abi_check("osk_layernorm_affine_bf16", weight.dtype == torch.float32, bias.dtype == torch.float32, x.stride(-1) == 1, out.stride(-1) == 1,
               x.stride(-2) % 8 == 0, out.stride(-2) % 8 == 0, x.stride(-2) >= C, out.stride(-2) >= C, _al(x, 16), _al(out, 16),
               _al(weight, 16), _al(bias, 16))
    assert out.shape == x.shape
    out.copy_(layernorm_affine_ref(x, weight, bias, eps).to(out.dtype))
    return out


def attention_causal(q, k, v, out, H, hd, scale):
    B, L, C = q.shape
    if hd != 64 or L > 4096:
        raise RuntimeError("osk_attention_causal_bf16 failed: status -2 (invalid argument / unsupported shape)")
    assert C == H * hd and k.shape == q.shape and v.shape == q.shape and out.shape == q.shape
    _abi_check("osk_attention_causal_bf16", *[t.stride(2) == 1 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and _al(t, 16)
                                               for t in (q, k, v)],
               out.stride(2) == 1, out.stride(0) % 4 == 0, out.stride(1) % 4 == 0, _al(out, 8))
    out.copy_(attention_causal_ref(q, k, v, H, hd, scale).to(out.dtype))
    return out


def gemm_quickgelu(a, w, bias, out):
    B, L, K = a.shape
    _abi_check("osk_gemm_quickgelu_bf16", K % 64 == 0, a.stride(2) == 1, a.stride(0) % 8 == 0, a.stride(1) % 8 == 0, w.stride(0) % 8 == 0,
               out.stride(0) % 4 == 0, out.stride(1) % 4 == 0, _al(a, 16), _al(w, 16), _al(out, 8), _al(bias, 16))
    assert tuple(out.shape) == (B, L, w.shape[0])
    out.copy_(gemm_quickgelu_ref(a, w, bias).to(out.dtype))
    return out
