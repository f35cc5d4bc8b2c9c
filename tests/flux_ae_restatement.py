"""TEST INFRASTRUCTURE ONLY -- the Flux 2-D autoencoder (reference opensora/models/vae/autoencoder_2d.py) restated as plain torch
functions over a state dict: the truth of the GPU tests (fp32) and their reference-precision comparator (the same code on bf16
tensors).  It runs wherever torch runs -- the reference tree is not needed.  tests/test_flux_ae_host.py pins it to the live
reference module (small geometry and shipped widths) and to the reference's output committed in tests/golden/flux_ae_small.npz.
Also the weights every Flux AE test uses: seeded, generated on the CPU, so every machine makes the same ones."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

SMALL = dict(ch=32, ch_mult=[1, 2, 2], num_res_blocks=2, z_channels=16, in_channels=3, out_ch=3)
SHIPPED = dict(ch=128, ch_mult=[1, 2, 4, 4], num_res_blocks=2, z_channels=16, in_channels=3, out_ch=3)
SCALE, SHIFT = 0.3611, 0.1159


def make_state_dict(model_or_shapes, seed: int = 0) -> dict:
    """seeded weights for the key set / shapes of a module (or a {key: shape} dict): conv weights N(0, 1/fan_in), GroupNorm scales
    1 + N(0, 0.1^2), every bias N(0, 0.05^2) -- f32, CPU"""
    shapes = model_or_shapes if isinstance(model_or_shapes, dict) else {k: v.shape for k, v in model_or_shapes.state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k in sorted(shapes):
        shp = tuple(shapes[k])
        x = torch.randn(shp, generator=g)
        if len(shp) == 4:
            x = x / math.sqrt(shp[1] * shp[2] * shp[3])
        elif "norm" in k and k.endswith(".weight"):
            x = 1.0 + 0.1 * x
        else:
            x = 0.05 * x
        sd[k] = x
    return {k: sd[k] for k in shapes}


_TORCH_CONV = [False]


def use_torch_conv(on: bool = True) -> None:
    """switch the restatement's convolutions to F.conv2d in the tensors' own dtype (the plain-PyTorch decoder a user would write:
    tools/flux_ae_time.py times it as the comparator).  Off (the default): the tap-matmul form below, the tests' truth."""
    _TORCH_CONV[0] = bool(on)


def _conv(sd, name, x, stride=1, padding=1):
    """nn.Conv2d as one f32 matmul per tap over the zero-padded input, rounded once to x's dtype (a bf16 conv's arithmetic: f32
    accumulate, one rounding).  Plain matmuls rather than F.conv2d, so that a fresh GPU box spends no time compiling convolution
    kernels for the truth."""
    if _TORCH_CONV[0]:
        return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], stride=stride, padding=padding)
    w, b = sd[name + ".weight"].float(), sd[name + ".bias"].float()
    k = w.shape[2]
    xp = F.pad(x.float(), (padding,) * 4)
    B, _, Hp, Wp = xp.shape
    Ho, Wo = (Hp - k) // stride + 1, (Wp - k) // stride + 1
    y = b.view(1, -1, 1, 1).expand(B, -1, Ho, Wo).contiguous()
    for dh in range(k):
        for dw in range(k):
            xt = xp[:, :, dh: dh + (Ho - 1) * stride + 1: stride, dw: dw + (Wo - 1) * stride + 1: stride]
            y += torch.einsum("bchw,oc->bohw", xt, w[:, :, dh, dw])
    return y.to(x.dtype)


def _gn(sd, name, x):
    return F.group_norm(x, 32, sd[name + ".weight"], sd[name + ".bias"], eps=1e-6)


def _resnet(sd, name, x):
    h = _conv(sd, name + ".conv1", F.silu(_gn(sd, name + ".norm1", x)))
    h = _conv(sd, name + ".conv2", F.silu(_gn(sd, name + ".norm2", h)))
    if name + ".nin_shortcut.weight" in sd:
        x = _conv(sd, name + ".nin_shortcut", x, padding=0)
    return x + h


def _attn(sd, name, x):
    h = _gn(sd, name + ".norm", x)
    q, k, v = (_conv(sd, f"{name}.{n}", h, padding=0) for n in ("q", "k", "v"))
    b, c, hh, ww = q.shape
    q, k, v = (t.reshape(b, 1, c, hh * ww).transpose(2, 3) for t in (q, k, v))
    o = F.scaled_dot_product_attention(q, k, v).transpose(2, 3).reshape(b, c, hh, ww)
    return x + _conv(sd, name + ".proj_out", o, padding=0)


def _mid(sd, name, x):
    return _resnet(sd, name + ".block_2", _attn(sd, name + ".attn_1", _resnet(sd, name + ".block_1", x)))


def decoder(sd: dict, cfg: dict, z: torch.Tensor) -> torch.Tensor:
    """Decoder.forward on NCHW z"""
    n = len(cfg["ch_mult"])
    h = _conv(sd, "decoder.conv_in", z)
    h = _mid(sd, "decoder.mid", h)
    for lvl in reversed(range(n)):
        for i in range(cfg["num_res_blocks"] + 1):
            h = _resnet(sd, f"decoder.up.{lvl}.block.{i}", h)
        if lvl != 0:
            h = _conv(sd, f"decoder.up.{lvl}.upsample.conv", F.interpolate(h, scale_factor=2.0, mode="nearest"))
    return _conv(sd, "decoder.conv_out", F.silu(_gn(sd, "decoder.norm_out", h)))


def encoder(sd: dict, cfg: dict, x: torch.Tensor) -> torch.Tensor:
    """Encoder.forward on NCHW x"""
    n = len(cfg["ch_mult"])
    h = _conv(sd, "encoder.conv_in", x)
    for lvl in range(n):
        for i in range(cfg["num_res_blocks"]):
            h = _resnet(sd, f"encoder.down.{lvl}.block.{i}", h)
        if lvl != n - 1:
            h = _conv(sd, f"encoder.down.{lvl}.downsample.conv", F.pad(h, (0, 1, 0, 1)), stride=2, padding=0)
    h = _mid(sd, "encoder.mid", h)
    return _conv(sd, "encoder.conv_out", F.silu(_gn(sd, "encoder.norm_out", h)))


def decode(sd: dict, cfg: dict, z: torch.Tensor) -> torch.Tensor:
    """AutoEncoder.decode: [B, C, T, h, w] latents -> [B, 3, T, 8h, 8w] in z's dtype (sd in the same dtype)"""
    B, C, T, h, w = z.shape
    z = z / SCALE + SHIFT
    x = decoder(sd, cfg, z.permute(0, 2, 1, 3, 4).reshape(B * T, C, h, w))
    return x.reshape(B, T, *x.shape[1:]).permute(0, 2, 1, 3, 4)


def encode_mode(sd: dict, cfg: dict, x: torch.Tensor) -> torch.Tensor:
    """AutoEncoder.encode with sample=False (the posterior mode), scaled and shifted"""
    B, C, T, H, W = x.shape
    p = encoder(sd, cfg, x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W))
    p = p.reshape(B, T, *p.shape[1:]).permute(0, 2, 1, 3, 4)
    mean = torch.chunk(p, 2, dim=1)[0]
    return SCALE * (mean - SHIFT)
