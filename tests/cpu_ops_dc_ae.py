"""TEST INFRASTRUCTURE ONLY -- tests/cpu_ops.py (the CPU emulation of the kernels' semantics) plus the entry points of the Video
DC-AE decoder (csrc/dc_ae.hip) with the Python call signatures of open_sora_amd/_C.py.  Never imported by the product path.
The `*_ref` functions are the formulas of include/osk.h in a chosen dtype before the output rounding; they run on any device
(f64 on the GPU for the kernel tests).  The table functions do the math in fp32 on the bf16-stored operands, rounded once."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.cpu_ops import *  # noqa: F401,F403  (the rest of the kernel table)
from tests.cpu_ops import _abi_check, _al


def conv3d_zp_ref(x, w, bias, ksize, up_t=False, up_hw=False, silu=False, res=None, dtype=torch.float32):
    """NDHWC in, NDHWC out: one matmul per tap over the explicitly zero-padded (and upsampled) input"""
    B, T, H, W, Cin = x.shape
    Cout = w.shape[0]
    taps = ksize ** 3
    assert float(w[:, taps * Cin:].float().abs().sum()) == 0.0, "weight K padding must be zero"
    wk = w[:, : taps * Cin].to(dtype).reshape(Cout, ksize, ksize, ksize, Cin)
    xs = x.to(dtype)
    if up_t:
        xs = xs.repeat_interleave(2, 1)
    if up_hw:
        xs = xs.repeat_interleave(2, 2).repeat_interleave(2, 3)
    To, Ho, Wo = xs.shape[1:4]
    p = ksize // 2
    xs = F.pad(xs, (0, 0, p, p, p, p, p, p))
    y = torch.zeros(B, To, Ho, Wo, Cout, dtype=dtype, device=x.device)
    for dt in range(ksize):
        for dh in range(ksize):
            for dw in range(ksize):
                y += xs[:, dt: dt + To, dh: dh + Ho, dw: dw + Wo, :] @ wk[:, dt, dh, dw, :].T
    if bias is not None:
        y = y + bias.to(dtype)
    if silu:
        y = y * torch.sigmoid(y)
    if res is not None:
        y = y + res.to(dtype)
    return y


def dup_shuffle_ref(x, Cout, ft, fhw):
    """the index formula of include/osk.h, as a gather"""
    B, T, H, W, Cin = x.shape
    rep = Cout * ft * fhw * fhw // Cin
    dev = x.device
    t = torch.arange(T * ft, device=dev).view(-1, 1, 1, 1)
    h = torch.arange(H * fhw, device=dev).view(1, -1, 1, 1)
    w = torch.arange(W * fhw, device=dev).view(1, 1, -1, 1)
    co = torch.arange(Cout, device=dev).view(1, 1, 1, -1)
    ci = (((co * ft + t % ft) * fhw + h % fhw) * fhw + w % fhw) // rep
    return x[:, t // ft, h // fhw, w // fhw, ci]


def dwconv3d_ref(x, w, bias, ksize, glu=False, dtype=torch.float32):
    B, T, H, W, C = x.shape
    p = ksize // 2
    xs = F.pad(x.to(dtype), (0, 0, p, p, p, p, p, p))
    wk = w.to(dtype).reshape(ksize, ksize, ksize, C)
    y = torch.zeros(B, T, H, W, C, dtype=dtype, device=x.device)
    for dt in range(ksize):
        for dh in range(ksize):
            for dw in range(ksize):
                y += xs[:, dt: dt + T, dh: dh + H, dw: dw + W, :] * wk[dt, dh, dw]
    if bias is not None:
        y = y + bias.to(dtype)
    if glu:
        a, g = y[..., : C // 2], y[..., C // 2:]
        y = a * (g * torch.sigmoid(g))
    return y


def gconv32_ref(x, w, dtype=torch.float32):
    C = x.shape[-1]
    xs = x.to(dtype).reshape(-1, C // 32, 32)
    return torch.einsum("mgi,goi->mgo", xs, w.to(dtype).reshape(C // 32, 32, 32)).reshape(x.shape)


def relu_linear_attn_ref(qkv, eps=1e-15, dtype=torch.float32):
    B, N, C3 = qkv.shape
    g = qkv.to(dtype).reshape(B, N, C3 // 96, 96).permute(0, 2, 1, 3)          # [B, G, N, 96]
    q, k, v = torch.relu(g[..., :32]), torch.relu(g[..., 32:64]), g[..., 64:]
    v1 = torch.cat([v, torch.ones_like(v[..., :1])], -1)                       # [B, G, N, 33]
    kv = v1.transpose(-1, -2) @ k                                              # [B, G, 33, 32]
    o = q @ kv.transpose(-1, -2)                                               # [B, G, N, 33]
    o = o[..., :32] / (o[..., 32:] + eps)
    return o.permute(0, 2, 1, 3).reshape(B, N, C3 // 3)


def rmsnorm_affine_ref(x, weight, bias, eps=1e-5, res=None, relu=False, dtype=torch.float32):
    xs = x.to(dtype)
    y = xs * torch.rsqrt(xs.square().mean(-1, keepdim=True) + eps) * weight.to(dtype) + bias.to(dtype)
    if relu:
        y = torch.relu(y)
    if res is not None:
        y = y + res.to(dtype)
    return y


# ---- the kernel table entries (signatures of open_sora_amd/_C.py)
def conv3d_zp(x, w, bias, out, ksize, up_t=False, up_hw=False, silu=False, res=None):
    B, T, H, W, Cin = x.shape
    _abi_check("osk_conv3d_zp_ndhwc_bf16", ksize in (1, 3), Cin % 8 == 0, Cin & (Cin - 1) == 0,
               w.shape[1] >= (ksize ** 3 * Cin + 63) // 64 * 64, _al(x, 16), _al(w, 16), _al(out, 8), x.is_contiguous(),
               out.is_contiguous())
    assert tuple(out.shape) == (B, T << int(up_t), H << int(up_hw), W << int(up_hw), w.shape[0])
    assert res is None or res.shape == out.shape
    out.copy_(conv3d_zp_ref(x, w, bias, ksize, up_t, up_hw, silu, res).to(out.dtype))
    return out


def dup_shuffle(x, out, ft, fhw):
    B, T, H, W, Cin = x.shape
    Cout = out.shape[-1]
    _abi_check("osk_dup_shuffle_ndhwc_bf16", ft in (1, 2), fhw in (1, 2), Cout % 8 == 0, (Cout * ft * fhw * fhw) % Cin == 0,
               _al(out, 16), x.is_contiguous(), out.is_contiguous())
    assert tuple(out.shape) == (B, T * ft, H * fhw, W * fhw, Cout)
    out.copy_(dup_shuffle_ref(x, Cout, ft, fhw))
    return out


def dwconv3d(x, w, bias, out, ksize, glu=False):
    C = x.shape[-1]
    _abi_check("osk_dwconv3d_ndhwc_bf16", ksize in (3, 5), C % (16 if glu else 8) == 0, tuple(w.shape) == (ksize ** 3, C),
               _al(x, 16), _al(w, 16), _al(out, 16), x.is_contiguous(), out.is_contiguous())
    assert tuple(out.shape) == tuple(x.shape[:-1]) + (C // 2 if glu else C,)
    out.copy_(dwconv3d_ref(x, w, bias, ksize, glu).to(out.dtype))
    return out


def gconv32(x, w, out):
    C = x.shape[-1]
    _abi_check("osk_gconv32_bf16", C % 32 == 0, tuple(w.shape) == (C, 32), _al(x, 16), _al(w, 16), _al(out, 16),
               x.is_contiguous(), out.is_contiguous())
    out.copy_(gconv32_ref(x, w).to(out.dtype))
    return out


def relu_linear_attn(qkv, out, eps=1e-15, workspace=None):
    B, N, C3 = qkv.shape
    _abi_check("osk_relu_linear_attn_bf16", C3 % 96 == 0, qkv.is_contiguous(), out.stride(2) == 1, out.stride(1) % 8 == 0,
               out.stride(0) == N * out.stride(1), _al(qkv, 16), _al(out, 16))
    out[:, :, : C3 // 3].copy_(relu_linear_attn_ref(qkv, eps).to(out.dtype))
    return out


def rmsnorm_affine(x, weight, bias, out, eps=1e-5, res=None, relu=False):
    C = x.shape[-1]
    _abi_check("osk_rmsnorm_affine_bf16", C % 8 == 0, weight.dtype == torch.float32, bias.dtype == torch.float32, _al(x, 16),
               _al(out, 16), x.is_contiguous(), out.is_contiguous())
    out.copy_(rmsnorm_affine_ref(x, weight, bias, eps, res, relu).to(out.dtype))
    return out
