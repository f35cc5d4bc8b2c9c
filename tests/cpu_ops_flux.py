"""TEST INFRASTRUCTURE ONLY -- tests/cpu_ops.py (the CPU emulation of the kernels' semantics) plus the entry point of the Flux
2-D autoencoder, osk_conv2d_nhwc_bf16, with the Python call signature of open_sora_amd/_C.py::conv2d.  Never imported by the
product path.  Math is fp32 on the bf16-stored operands (f64 with `exact=True` in the emulation tests), output rounded once."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.cpu_ops import *  # noqa: F401,F403  (the rest of the kernel table)
from tests.cpu_ops import _abi_check, _al


def conv2d_ref(x, w, bias, ksize, stride=1, pad=1, up=False, res=None, Ho=None, Wo=None, dtype=torch.float32):
    """the arithmetic of osk_conv2d_nhwc_bf16 in `dtype`, before the output rounding: NHWC in, NHWC out.  A sum of one matmul per
    tap over explicitly zero-padded input, so it runs in any dtype on any device (f64 on the GPU for the kernel tests)."""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    taps = ksize * ksize
    assert float(w[:, taps * Cin:].float().abs().sum()) == 0.0, "weight K padding must be zero"
    wk = w[:, : taps * Cin].to(dtype).reshape(Cout, ksize, ksize, Cin)
    xs = x.to(dtype)
    if up:
        xs = xs.repeat_interleave(2, 1).repeat_interleave(2, 2)
    Hu, Wu = xs.shape[1], xs.shape[2]
    Ho = Ho if Ho is not None else (Hu + 2 * pad - ksize) // stride + 1
    Wo = Wo if Wo is not None else (Wu + 2 * pad - ksize) // stride + 1
    # zeros in front (pad) and as many behind as the output extent reads
    far_h = max(0, (Ho - 1) * stride + ksize - pad - Hu)
    far_w = max(0, (Wo - 1) * stride + ksize - pad - Wu)
    xs = F.pad(xs, (0, 0, pad, far_w, pad, far_h))
    y = torch.zeros(B, Ho, Wo, Cout, dtype=dtype, device=x.device)
    for dh in range(ksize):
        for dw in range(ksize):
            xt = xs[:, dh: dh + (Ho - 1) * stride + 1: stride, dw: dw + (Wo - 1) * stride + 1: stride, :]
            y += xt @ wk[:, dh, dw, :].T
    if bias is not None:
        y = y + bias.to(dtype)
    if res is not None:
        y = y + res.to(dtype)
    return y


def conv2d(x, w, bias, out, ksize, stride=1, pad=1, up=False, res=None):
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = out.shape[1], out.shape[2]
    Hu, Wu = (2 * H, 2 * W) if up else (H, W)
    _abi_check("osk_conv2d_nhwc_bf16", ksize in (1, 3), stride in (1, 2), 0 <= pad < ksize, Cin % 8 == 0, Cin & (Cin - 1) == 0,
               w.shape[1] >= (ksize * ksize * Cin + 63) // 64 * 64, (Ho - 1) * stride - pad <= Hu - 1,
               (Wo - 1) * stride - pad <= Wu - 1, _al(x, 16), _al(w, 16), _al(out, 8), x.is_contiguous(), out.is_contiguous())
    assert tuple(out.shape) == (B, Ho, Wo, Cout) and (res is None or res.shape == out.shape)
    out.copy_(conv2d_ref(x, w, bias, ksize, stride, pad, up, res, Ho, Wo).to(out.dtype))
    return out
