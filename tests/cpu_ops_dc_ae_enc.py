"""TEST INFRASTRUCTURE ONLY -- tests/cpu_ops_dc_ae.py (the CPU emulation of the Video DC-AE decoder's kernel table) plus the two
entry points the ENCODER adds (csrc/dc_ae.hip: osk_conv3d_zp_strided_ndhwc_bf16, osk_unshuffle_avg_ndhwc_bf16), with the Python
call signatures of open_sora_amd/_C.py.  Never imported by the product path.  As there, the `*_ref` functions are the formulas of
include/osk.h in a chosen dtype before the output rounding and run on any device; the table functions do the math in fp32 on the
bf16-stored operands, rounded once."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.cpu_ops_dc_ae import *  # noqa: F401,F403  (the decoder's kernel table)
from tests.cpu_ops_dc_ae import _abi_check, _al


def conv3d_zp_strided_ref(x, w, bias, stride_t, stride_hw=2, res=None, dtype=torch.float32):
    """NDHWC in, NDHWC out: one matmul per tap over strided windows of the explicitly zero-padded input"""
    B, T, H, W, Cin = x.shape
    Cout = w.shape[0]
    assert float(w[:, 27 * Cin:].float().abs().sum()) == 0.0, "weight K padding must be zero"
    wk = w[:, : 27 * Cin].to(dtype).reshape(Cout, 3, 3, 3, Cin)
    To, Ho, Wo = (T - 1) // stride_t + 1, (H - 1) // stride_hw + 1, (W - 1) // stride_hw + 1
    xs = F.pad(x.to(dtype), (0, 0, 1, 1, 1, 1, 1, 1))
    y = torch.zeros(B, To, Ho, Wo, Cout, dtype=dtype, device=x.device)
    for dt in range(3):
        for dh in range(3):
            for dw in range(3):
                win = xs[:, dt: dt + (To - 1) * stride_t + 1: stride_t, dh: dh + (Ho - 1) * stride_hw + 1: stride_hw,
                         dw: dw + (Wo - 1) * stride_hw + 1: stride_hw, :]
                y += win @ wk[:, dt, dh, dw, :].T
    if bias is not None:
        y = y + bias.to(dtype)
    if res is not None:
        y = y + res.to(dtype)
    return y


def unshuffle_avg_ref(x, Cout, ft, fhw, dtype=torch.float32):
    """the index formula of include/osk.h, as a gather and a sum over g"""
    B, T, H, W, Cin = x.shape
    per = ft * fhw * fhw
    gs = Cin * per // Cout
    dev = x.device
    t = torch.arange(T // ft, device=dev).view(-1, 1, 1, 1, 1)
    h = torch.arange(H // fhw, device=dev).view(1, -1, 1, 1, 1)
    w = torch.arange(W // fhw, device=dev).view(1, 1, -1, 1, 1)
    u = torch.arange(Cout, device=dev).view(1, 1, 1, -1, 1) * gs + torch.arange(gs, device=dev).view(1, 1, 1, 1, -1)
    c, s = u // per, u % per
    dt, dh, dw = s // (fhw * fhw), (s // fhw) % fhw, s % fhw
    return x.to(dtype)[:, t * ft + dt, h * fhw + dh, w * fhw + dw, c].sum(-1) / gs


# ---- the kernel table entries (signatures of open_sora_amd/_C.py)
def conv3d_zp_strided(x, w, bias, out, stride_t, res=None):
    B, T, H, W, Cin = x.shape
    _abi_check("osk_conv3d_zp_strided_ndhwc_bf16", stride_t in (1, 2), Cin % 8 == 0, Cin & (Cin - 1) == 0,
               w.shape[1] >= (27 * Cin + 63) // 64 * 64, _al(x, 16), _al(w, 16), _al(out, 8), x.is_contiguous(), out.is_contiguous())
    assert tuple(out.shape) == (B, (T - 1) // stride_t + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1, w.shape[0])
    assert res is None or res.shape == out.shape
    out.copy_(conv3d_zp_strided_ref(x, w, bias, stride_t, 2, res).to(out.dtype))
    return out


def unshuffle_avg(x, out, ft, fhw):
    B, T, H, W, Cin = x.shape
    Cout = out.shape[-1]
    _abi_check("osk_unshuffle_avg_ndhwc_bf16", ft in (1, 2), fhw in (1, 2), Cout % 8 == 0, (Cin * ft * fhw * fhw) % Cout == 0,
               T % ft == 0, H % fhw == 0, W % fhw == 0, _al(out, 16), x.is_contiguous(), out.is_contiguous())
    assert tuple(out.shape) == (B, T // ft, H // fhw, W // fhw, Cout)
    out.copy_(unshuffle_avg_ref(x, Cout, ft, fhw).to(out.dtype))
    return out
