"""TEST INFRASTRUCTURE ONLY -- tests/cpu_ops_dc_ae.py (the CPU emulation of the kernel table, with osk_rmsnorm_affine_bf16) plus the
entry points the T5 text encoder uses that the table lacked: osk_attention_relbias_bf16 (csrc/attention_relbias.hip) and
osk_gemm_geglu_bf16 (its weight packing is the product's own host function), with the Python call signatures of
open_sora_amd/_C.py.  Never imported by the product path.  `attention_relbias_ref` is the formula of include/osk.h in a chosen dtype before the output rounding and runs on any device;
the table functions do the math in fp32 on the bf16-stored operands, rounded once."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.cpu_ops_dc_ae import *  # noqa: F401,F403  (the rest of the kernel table)
from tests.cpu_ops_dc_ae import _abi_check, _al


def attention_relbias_ref(q, k, v, H, hd, scale, bias=None, dtype=torch.float32):
    """out[b, i, h] = sum_j softmax_j(scale q_i . k_j + bias[h, (j - i) + L - 1]) v_j;  q, k, v [B, L, H * hd], bias [H, >= 2 L - 1].
    Every operation in `dtype` (bf16: a reference-precision evaluation that materialises and rounds the scores)."""
    B, L, _ = q.shape
    qh, kh, vh = (t.to(dtype).reshape(B, L, H, hd).transpose(1, 2) for t in (q, k, v))
    s = (qh @ kh.transpose(2, 3)) * scale
    if bias is not None:
        idx = torch.arange(L, device=q.device)[None, :] - torch.arange(L, device=q.device)[:, None] + (L - 1)
        s = s + bias.to(dtype)[:, idx]
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, L, H * hd)


# ---- the kernel table entries (signatures of open_sora_amd/_C.py)
def attention_relbias(q, k, v, out, H, hd, scale, bias=None):
    B, L, C = q.shape
    if hd != 64 or L > 4096:
        raise RuntimeError("osk_attention_relbias_bf16 failed: status -2 (invalid argument / unsupported shape)")
    assert C == H * hd and k.shape == q.shape and v.shape == q.shape and out.shape == q.shape
    _abi_check("osk_attention_relbias_bf16", *[t.stride(2) == 1 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and _al(t, 16)
                                                for t in (q, k, v)],
               out.stride(2) == 1, out.stride(0) % 4 == 0, out.stride(1) % 4 == 0, _al(out, 8),
               bias is None or (bias.dtype == torch.float32 and bias.shape[0] == H and bias.stride(1) == 1 and bias.stride(0) >= 2 * L - 1
                                and bias.shape[1] >= 2 * L - 1))
    out.copy_(attention_relbias_ref(q, k, v, H, hd, scale, bias).to(out.dtype))
    return out


def geglu_pack(w_value, w_gate, b_value=None, b_gate=None):
    """open_sora_amd/_C.py::geglu_pack itself: the packing is host-side torch code, not a kernel"""
    from open_sora_amd._C import geglu_pack as pack

    return pack(w_value, w_gate, b_value, b_gate)


def gemm_geglu(a, w_packed, bias_packed, out, workspace=None):
    """out = value * gelu_tanh(gate) of the packed projection; un-packs the rows by the rule of include/osk.h"""
    B, L, K = a.shape
    n_out = w_packed.shape[0] // 2
    _abi_check("osk_gemm_geglu_bf16", n_out % 16 == 0, K % 64 == 0, a.stride(2) == 1, a.stride(0) % 8 == 0, a.stride(1) % 8 == 0,
               w_packed.stride(0) % 8 == 0, out.stride(0) % 4 == 0, out.stride(1) % 4 == 0, _al(a, 16), _al(w_packed, 16), _al(out, 8))
    if B * L < 256 or 2 * n_out < 128:     # off the 256 x 256 tile path: the library needs the workspace
        if workspace is None or workspace.numel() * workspace.element_size() < B * L * 2 * n_out * 2:
            raise RuntimeError("osk_gemm_geglu_bf16 failed: status -2 (invalid argument / unsupported shape)")
    assert out.shape == (B, L, n_out)
    y = a.float() @ w_packed.float().T
    if bias_packed is not None:
        y = y + bias_packed.float()
    y = y.reshape(B, L, n_out // 16, 2, 16)
    out.copy_((y[..., 0, :] * F.gelu(y[..., 1, :], approximate="tanh")).reshape(B, L, n_out).to(out.dtype))
    return out
