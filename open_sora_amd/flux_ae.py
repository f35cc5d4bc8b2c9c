"""MI355X-native Flux 2-D autoencoder (the image stage of the reference's t2i2v pipeline) behind the reference's module API.

Mirrors, by name, call signature and state-dict keys (so `flux1-dev-ae.safetensors` loads unchanged):
    AutoEncoderConfig / AttnBlock / ResnetBlock / Downsample / Upsample / Encoder / Decoder / AutoEncoder / AutoEncoderFlux
                                                 /root/reference/opensora/models/vae/autoencoder_2d.py:32-339
    DiagonalGaussianDistribution                 /root/reference/opensora/models/vae/utils.py:112-150

The nn.Modules only HOLD parameters.  All arithmetic runs in the gfx950 kernels of include/osk.h through the kernel table
(mmdit.ops()); there is no eager fallback.  Activations are kept channels-last (NHWC bf16, frames folded into the batch as the
reference does) between the two boundary conversions.  Every convolution is osk_conv2d_nhwc_bf16: the zero padding, the nearest
upsample of Upsample, the explicit (0, 1, 0, 1) pad of Downsample and the residual add of ResnetBlock are folded into it.  GroupNorm
and the mid-block attention are the causal VAE's kernels (hunyuan_vae._gn / _one_head_attention with one frame).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
from torch import Tensor, nn

from . import hunyuan_vae as _hv
from .hunyuan_vae import BF16, _gn, _ops, _pad8, _plan

# =============================================================================================
# parameter containers (names == reference state-dict keys)
# =============================================================================================


@dataclass
class AutoEncoderConfig:
    """Field-for-field autoencoder_2d.py:32-45."""

    from_pretrained: str | None
    cache_dir: str | None
    resolution: int
    in_channels: int
    ch: int
    out_ch: int
    ch_mult: list[int]
    num_res_blocks: int
    z_channels: int
    scale_factor: float
    shift_factor: float
    sample: bool = True


class _Holder(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover - guard
        raise RuntimeError(f"{type(self).__name__} holds parameters only; its arithmetic runs in libosk_hip.so "
                           "(AutoEncoder.encode/decode); there is no eager fallback.")


def _norm(c: int) -> nn.GroupNorm:
    return nn.GroupNorm(num_groups=32, num_channels=c, eps=1e-6, affine=True)


class AttnBlock(_Holder):
    """autoencoder_2d.py:48-72"""

    def __init__(self, in_channels: int):
        super().__init__()
        self.norm = _norm(in_channels)
        self.q = nn.Conv2d(in_channels, in_channels, kernel_size=1)
        self.k = nn.Conv2d(in_channels, in_channels, kernel_size=1)
        self.v = nn.Conv2d(in_channels, in_channels, kernel_size=1)
        self.proj_out = nn.Conv2d(in_channels, in_channels, kernel_size=1)


class ResnetBlock(_Holder):
    """autoencoder_2d.py:75-101"""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.in_channels = in_channels
        out_channels = in_channels if out_channels is None else out_channels
        self.out_channels = out_channels
        self.norm1 = _norm(in_channels)
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.norm2 = _norm(out_channels)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1)
        if self.in_channels != self.out_channels:
            self.nin_shortcut = nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=1, padding=0)


class Downsample(_Holder):
    """autoencoder_2d.py:104-113 (F.pad (0, 1, 0, 1) with zeros, then an unpadded stride-2 3 x 3 conv)"""

    def __init__(self, in_channels: int):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=2, padding=0)


class Upsample(_Holder):
    """autoencoder_2d.py:115-122 (nearest 2x, then a padding=1 3 x 3 conv)"""

    def __init__(self, in_channels: int):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1)


class Encoder(_Holder):
    """autoencoder_2d.py:125-191"""

    def __init__(self, config: AutoEncoderConfig):
        super().__init__()
        self.ch = config.ch
        self.num_resolutions = len(config.ch_mult)
        self.num_res_blocks = config.num_res_blocks
        self.resolution = config.resolution
        self.in_channels = config.in_channels
        self.conv_in = nn.Conv2d(config.in_channels, self.ch, kernel_size=3, stride=1, padding=1)
        in_ch_mult = (1,) + tuple(config.ch_mult)
        self.in_ch_mult = in_ch_mult
        self.down = nn.ModuleList()
        block_in = self.ch
        for i_level in range(self.num_resolutions):
            block = nn.ModuleList()
            attn = nn.ModuleList()
            block_in = config.ch * in_ch_mult[i_level]
            block_out = config.ch * config.ch_mult[i_level]
            for _ in range(self.num_res_blocks):
                block.append(ResnetBlock(in_channels=block_in, out_channels=block_out))
                block_in = block_out
            down = nn.Module()
            down.block = block
            down.attn = attn
            if i_level != self.num_resolutions - 1:
                down.downsample = Downsample(block_in)
            self.down.append(down)
        self.mid = nn.Module()
        self.mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in)
        self.mid.attn_1 = AttnBlock(block_in)
        self.mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in)
        self.norm_out = _norm(block_in)
        self.conv_out = nn.Conv2d(block_in, 2 * config.z_channels, kernel_size=3, stride=1, padding=1)


class Decoder(_Holder):
    """autoencoder_2d.py:194-258"""

    def __init__(self, config: AutoEncoderConfig):
        super().__init__()
        self.ch = config.ch
        self.num_resolutions = len(config.ch_mult)
        self.num_res_blocks = config.num_res_blocks
        self.resolution = config.resolution
        self.in_channels = config.in_channels
        self.ffactor = 2 ** (self.num_resolutions - 1)
        block_in = config.ch * config.ch_mult[self.num_resolutions - 1]
        curr_res = config.resolution // 2 ** (self.num_resolutions - 1)
        self.z_shape = (1, config.z_channels, curr_res, curr_res)
        self.conv_in = nn.Conv2d(config.z_channels, block_in, kernel_size=3, stride=1, padding=1)
        self.mid = nn.Module()
        self.mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in)
        self.mid.attn_1 = AttnBlock(block_in)
        self.mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in)
        self.up = nn.ModuleList()
        for i_level in reversed(range(self.num_resolutions)):
            block = nn.ModuleList()
            attn = nn.ModuleList()
            block_out = config.ch * config.ch_mult[i_level]
            for _ in range(self.num_res_blocks + 1):
                block.append(ResnetBlock(in_channels=block_in, out_channels=block_out))
                block_in = block_out
            up = nn.Module()
            up.block = block
            up.attn = attn
            if i_level != 0:
                up.upsample = Upsample(block_in)
            self.up.insert(0, up)  # prepend to get consistent order
        self.norm_out = _norm(block_in)
        self.conv_out = nn.Conv2d(block_in, config.out_ch, kernel_size=3, stride=1, padding=1)


class DiagonalGaussianDistribution:
    """vae/utils.py:112-150 (small latent-sized tensors: plain torch on the device)."""

    def __init__(self, parameters: Tensor, deterministic: bool = False):
        self.parameters = parameters
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.deterministic = deterministic
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)
        if self.deterministic:
            self.var = self.std = torch.zeros_like(self.mean).to(device=self.parameters.device, dtype=self.mean.dtype)

    def sample(self) -> Tensor:
        return self.mean + self.std * torch.randn(self.mean.shape).to(device=self.parameters.device, dtype=self.mean.dtype)

    def kl(self, other=None) -> Tensor:
        if self.deterministic:
            return torch.Tensor([0.0])
        if other is None:
            return 0.5 * torch.sum(torch.pow(self.mean, 2) + self.var - 1.0 - self.logvar, dim=[1, 3, 4]).flatten(0)
        return 0.5 * torch.sum(torch.pow(self.mean - other.mean, 2) / other.var + self.var / other.var - 1.0 - self.logvar
                               + other.logvar, dim=[1, 3, 4]).flatten(0)

    def mode(self) -> Tensor:
        return self.mean


# =============================================================================================
# engine: kernels over NHWC tensors
# =============================================================================================
class _Conv2dPlan:
    """weight [Cout, Cin, k, k] -> bf16 [Cout, round_up(k^2 * Cin_p, 64)], K = tap-major / channel-minor, Cin zero-padded to
    8 * 2^j; bias f32 (osk_conv2d_nhwc_bf16's operands)."""

    def __init__(self, conv: nn.Conv2d):
        w = conv.weight.detach()
        co, ci, k = w.shape[0], w.shape[1], w.shape[2]
        cip = _pad8(ci)
        wk = torch.zeros(co, k, k, cip, dtype=BF16, device=w.device)
        wk[..., :ci] = w.permute(0, 2, 3, 1).to(BF16)
        K = k * k * cip
        Kp = (K + 63) // 64 * 64
        self.w = torch.zeros(co, Kp, dtype=BF16, device=w.device)
        self.w[:, :K] = wk.reshape(co, K)
        self.b = None if conv.bias is None else conv.bias.detach().float().contiguous()
        self.cin, self.cin_p, self.cout, self.k = ci, cip, co, k
        self.stride = conv.stride[0]
        self.pad = conv.padding[0]


def conv2d_out_dims(H: int, W: int, ksize: int = 3, stride: int = 1, pad: int = 1, up: bool = False, pad_far: int | None = None):
    """output extent of a conv with `pad` zero rows in front and `pad_far` (default: pad) behind the (upsampled) image"""
    Hu, Wu = (2 * H, 2 * W) if up else (H, W)
    pf = pad if pad_far is None else pad_far
    return (Hu + pad + pf - ksize) // stride + 1, (Wu + pad + pf - ksize) // stride + 1


def _conv(mod: nn.Conv2d, x: Tensor, up: bool = False, res: Tensor | None = None, pad_far: int | None = None) -> Tensor:
    p = _plan(mod, "conv2d")
    B, H, W, C = x.shape
    assert C == p.cin_p, (C, p.cin_p)
    Ho, Wo = conv2d_out_dims(H, W, p.k, p.stride, p.pad, up, pad_far)
    out = torch.empty(B, Ho, Wo, p.cout, dtype=BF16, device=x.device)
    return _ops().conv2d(x, p.w, p.b, out, p.k, p.stride, p.pad, up, res)


def _resnet(blk: ResnetBlock, x: Tensor) -> Tensor:
    """ResnetBlock.forward (autoencoder_2d.py:89-101); the residual add rides in conv2's epilogue."""
    h = _conv(blk.conv1, _gn(blk.norm1, x, True))
    sc = _conv(blk.nin_shortcut, x) if blk.in_channels != blk.out_channels else x
    return _conv(blk.conv2, _gn(blk.norm2, h, True), res=sc)


def _attn(att: AttnBlock, x: Tensor) -> Tensor:
    """AttnBlock.forward (autoencoder_2d.py:56-72): one head of dim C over the H x W tokens of each image (one frame)."""
    B, H, W, C = x.shape
    return _hv._one_head_attention(x.view(B, 1, H, W, C), att.norm, att.q, att.k, att.v, att.proj_out).view(B, H, W, C)


def _mid(mid: nn.Module, x: Tensor) -> Tensor:
    return _resnet(mid.block_2, _attn(mid.attn_1, _resnet(mid.block_1, x)))


def run_encoder(enc: Encoder, x: Tensor) -> Tensor:
    """Encoder.forward (autoencoder_2d.py:165-191) on NHWC input (channels padded to 8)."""
    h = _conv(enc.conv_in, x)
    for i_level in range(enc.num_resolutions):
        for i_block in range(enc.num_res_blocks):
            h = _resnet(enc.down[i_level].block[i_block], h)
        if i_level != enc.num_resolutions - 1:
            h = _conv(enc.down[i_level].downsample.conv, h, pad_far=1)   # F.pad (0, 1, 0, 1) + stride 2
    h = _mid(enc.mid, h)
    return _conv(enc.conv_out, _gn(enc.norm_out, h, True))


def run_decoder(dec: Decoder, z: Tensor) -> Tensor:
    """Decoder.forward (autoencoder_2d.py:234-258) on NHWC input; the nearest upsample is folded into the upsampler conv."""
    h = _conv(dec.conv_in, z)
    h = _mid(dec.mid, h)
    for i_level in reversed(range(dec.num_resolutions)):
        for i_block in range(dec.num_res_blocks + 1):
            h = _resnet(dec.up[i_level].block[i_block], h)
        if i_level != 0:
            h = _conv(dec.up[i_level].upsample.conv, h, up=True)
    return _conv(dec.conv_out, _gn(dec.norm_out, h, True))


def _to_nhwc(x: Tensor) -> Tensor:
    """[B, C, T, H, W] -> bf16 [(B T), H, W, C_pad] (channels zero-padded to 8 * 2^j)"""
    B, C, T, H, W = x.shape
    cp = _pad8(C)
    out = torch.zeros(B, T, H, W, cp, dtype=BF16, device=x.device) if cp != C else \
        torch.empty(B, T, H, W, C, dtype=BF16, device=x.device)
    out[..., :C].copy_(x.permute(0, 2, 3, 4, 1))
    return out.view(B * T, H, W, cp)


def _to_ncthw(x: Tensor, B: int, dtype) -> Tensor:
    """[(B T), H, W, C] -> [B, C, T, H, W] in dtype"""
    BT, H, W, C = x.shape
    return x.view(B, BT // B, H, W, C).permute(0, 4, 1, 2, 3).contiguous().to(dtype)


# =============================================================================================
# the model
# =============================================================================================
class AutoEncoder(nn.Module):
    """autoencoder_2d.py:261-303"""

    def __init__(self, config: AutoEncoderConfig):
        super().__init__()
        self.encoder = Encoder(config)
        self.decoder = Decoder(config)
        self.scale_factor = config.scale_factor
        self.shift_factor = config.shift_factor
        self.sample = config.sample

    def encode_(self, x: Tensor) -> tuple[Tensor, DiagonalGaussianDistribution]:
        params = _to_ncthw(run_encoder(self.encoder, _to_nhwc(x)), x.shape[0], x.dtype)
        posterior = DiagonalGaussianDistribution(params)
        z = posterior.sample() if self.sample else posterior.mode()
        z = self.scale_factor * (z - self.shift_factor)
        return z, posterior

    def encode(self, x: Tensor) -> Tensor:
        return self.encode_(x)[0]

    def decode(self, z: Tensor) -> Tensor:
        z = z / self.scale_factor + self.shift_factor
        return _to_ncthw(run_decoder(self.decoder, _to_nhwc(z)), z.shape[0], z.dtype)

    def forward(self, x: Tensor) -> tuple[Tensor, DiagonalGaussianDistribution, Tensor]:
        z, posterior = self.encode_(x)
        return self.decode(z), posterior, z

    def get_last_layer(self):
        return self.decoder.conv_out.weight


def AutoEncoderFlux(
    from_pretrained: str,
    cache_dir=None,
    resolution=256,
    in_channels=3,
    ch=128,
    out_ch=3,
    ch_mult=[1, 2, 4, 4],
    num_res_blocks=2,
    z_channels=16,
    scale_factor=0.3611,
    shift_factor=0.1159,
    device_map: str | torch.device = "cuda",
    torch_dtype: torch.dtype = torch.bfloat16,
) -> AutoEncoder:
    """autoencoder_2d.py:306-339 (registered there as "autoencoder_2d").

    The activations between layers are fed to osk_conv2d_nhwc_bf16 and the GroupNorm kernels as they are, so every width
    ch * ch_mult[i] must be 8 * 2^j in 32 .. 512 (every Flux AE configuration is); the 3-channel image and the z_channels latent
    are zero-padded to the next 8 * 2^j at the module boundary.  Other widths raise ValueError here."""
    for m in [1] + list(ch_mult):
        c = ch * m
        if c < 32 or c > 512 or c & (c - 1):
            raise ValueError(f"flux_ae: channel width ch * ch_mult = {ch} * {m} = {c} is not 8 * 2^j in 32 .. 512 "
                             "(osk_conv2d_nhwc_bf16 / osk_groupnorm_*_ndhwc_bf16 shapes)")
    config = AutoEncoderConfig(from_pretrained=from_pretrained, cache_dir=cache_dir, resolution=resolution,
                               in_channels=in_channels, ch=ch, out_ch=out_ch, ch_mult=list(ch_mult),
                               num_res_blocks=num_res_blocks, z_channels=z_channels, scale_factor=scale_factor,
                               shift_factor=shift_factor)
    with torch.device(device_map):
        model = AutoEncoder(config).to(torch_dtype)
    if from_pretrained:
        from .ckpt import load_checkpoint
        model = load_checkpoint(model, from_pretrained, cache_dir=cache_dir, device_map=device_map)
    return model
