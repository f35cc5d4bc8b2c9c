"""MI355X-native Video DC-AE (the autoencoder of the reference's high-compression pipeline, "dc-ae-f32t4c128": 32x spatial,
4x temporal, 128 latent channels) behind the reference's module API: the decoder always, the encoder on request.

Mirrors, by name, call signature and `encoder.*` / `decoder.*` state-dict keys:
    EncoderConfig / DecoderConfig / DCAEConfig / Encoder / Decoder / DCAE / dc_ae_f32   /root/reference/opensora/models/dc_ae/models/dc_ae.py
    ConvLayer / InterpolateConvUpSampleLayer / ChannelDuplicatingPixelShuffleUpSampleLayer /
    PixelUnshuffleChannelAveragingDownSampleLayer / GLUMBConv / ResBlock / LiteMLA /
    EfficientViTBlock / ResidualBlock / OpSequential / IdentityLayer             .../dc_ae/models/nn/ops.py
    RMSNorm3d                                                                    .../dc_ae/models/nn/norm.py:63-68
    DC_AE                                                                        .../dc_ae/ae_model_zoo.py:52-85

The nn.Modules only HOLD parameters.  All arithmetic runs in the gfx950 kernels of include/osk.h (csrc/dc_ae.hip + osk_gemm_bf16 +
osk_blend_bf16) through the kernel table (mmdit.ops()); there is no eager fallback.  Activations are channels-last (NDHWC bf16)
between the two boundary conversions of one `_decode` / `_encode` call.

The encoder is opt-in (`DCAEConfig.build_encoder`, or the factory `DC_AE_with_encoder`): text-to-video inference needs `decode`
alone.  Without it `DCAE.encode` / `forward` raise NotImplementedError, the module has no `encoder` sub-module, and
`load_state_dict` drops the `encoder.*` keys of a full checkpoint (everything else is strict).  With it the module holds both
halves in the reference's order and loads both strictly.

Fusion choices (DESIGN.md section 4 has the table):
  - zero padding, the nearest upsample (T and H,W independently), the downsample stride, bias, SiLU and the `main + shortcut` add:
    inside the conv kernel;
  - the pixel-unshuffle channel-averaging shortcut of the encoder: a gather kernel of its own that produces the conv's `res`
    operand, for the reason given for the decoder's shortcut next;
  - the channel-duplicating pixel-shuffle shortcut: a gather kernel of its own that produces the conv's `res` operand (the gathered
    channel depends on the output voxel's parity, so folding it into the conv epilogue would cost a scalar gather per accumulator
    lane; as a separate pass it is one read of the small block input and one write);
  - GLU (x * silu(gate)) and the bias: inside the depthwise conv;
  - ReLU of project_out and the identity-shortcut add of ResidualBlock: inside the RMSNorm kernel.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Optional

import torch
from torch import Tensor, nn

from .hunyuan_vae import BF16, _ops

# =============================================================================================
# configuration (dc_ae.py:47-112), plain dataclasses
# =============================================================================================


@dataclass
class EncoderConfig:
    """dc_ae.py:47-64"""

    in_channels: int = 3
    latent_channels: int = 32
    width_list: tuple = (128, 256, 512, 512, 1024, 1024)
    depth_list: tuple = (2, 2, 2, 2, 2, 2)
    block_type: Any = "ResBlock"
    norm: str = "rms2d"
    act: str = "silu"
    downsample_block_type: str = "ConvPixelUnshuffle"
    downsample_match_channel: bool = True
    downsample_shortcut: Optional[str] = "averaging"
    out_norm: Optional[str] = None
    out_act: Optional[str] = None
    out_shortcut: Optional[str] = "averaging"
    double_latent: bool = False
    is_video: bool = False
    temporal_downsample: tuple = ()


@dataclass
class DecoderConfig:
    """dc_ae.py:67-83"""

    in_channels: int = 3
    latent_channels: int = 32
    in_shortcut: Optional[str] = "duplicating"
    width_list: tuple = (128, 256, 512, 512, 1024, 1024)
    depth_list: tuple = (2, 2, 2, 2, 2, 2)
    block_type: Any = "ResBlock"
    norm: Any = "rms2d"
    act: Any = "silu"
    upsample_block_type: str = "ConvPixelShuffle"
    upsample_match_channel: bool = True
    upsample_shortcut: str = "duplicating"
    out_norm: str = "rms2d"
    out_act: str = "relu"
    is_video: bool = False
    temporal_upsample: tuple = ()


@dataclass
class DCAEConfig:
    """dc_ae.py:86-112"""

    in_channels: int = 3
    latent_channels: int = 32
    time_compression_ratio: int = 1
    spatial_compression_ratio: int = 32
    encoder: EncoderConfig = field(default_factory=EncoderConfig)
    decoder: DecoderConfig = field(default_factory=DecoderConfig)
    use_quant_conv: bool = False
    pretrained_path: Optional[str] = None
    pretrained_source: str = "dc-ae"
    scaling_factor: Optional[float] = None
    is_image_model: bool = False
    is_training: bool = False
    use_spatial_tiling: bool = False
    use_temporal_tiling: bool = False
    spatial_tile_size: int = 256
    temporal_tile_size: int = 32
    tile_overlap_factor: float = 0.25
    build_encoder: bool = False    # not a reference field: this package builds the encoder half only on request


def dc_ae_f32(name: str, pretrained_path: Optional[str]) -> DCAEConfig:
    """dc_ae.py:790-814, the values of its dotlist as plain dataclasses"""
    if name not in ("dc-ae-f32t4c128",):
        raise NotImplementedError(name)
    blocks = ["ResBlock", "ResBlock", "ResBlock", "EViTS5_GLU", "EViTS5_GLU", "EViTS5_GLU"]
    widths = (128, 256, 512, 512, 1024, 1024)
    temporal = (False, False, False, True, True, False)
    enc = EncoderConfig(in_channels=3, latent_channels=128, block_type=list(blocks), width_list=widths, depth_list=(2, 2, 2, 3, 3, 3),
                        downsample_block_type="Conv", norm="rms3d", is_video=True, temporal_downsample=temporal)
    dec = DecoderConfig(in_channels=3, latent_channels=128, block_type=list(blocks), width_list=widths, depth_list=(3, 3, 3, 3, 3, 3),
                        upsample_block_type="InterpolateConv", norm="rms3d", act="silu", out_norm="rms3d", is_video=True,
                        temporal_upsample=temporal)
    return DCAEConfig(in_channels=3, latent_channels=128, time_compression_ratio=4, spatial_compression_ratio=32, encoder=enc,
                      decoder=dec, pretrained_path=pretrained_path)


# =============================================================================================
# parameter containers (names == reference state-dict keys)
# =============================================================================================
class _Holder(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover - guard
        raise RuntimeError(f"{type(self).__name__} holds parameters only; its arithmetic runs in libosk_hip.so (DCAE.decode); "
                           "there is no eager fallback.")


class RMSNorm3d(_Holder):
    """nn/norm.py:38-68"""

    def __init__(self, num_features: int, eps: float = 1e-5):
        super().__init__()
        self.num_features, self.eps = num_features, eps
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))


class IdentityLayer(_Holder):
    """ops.py:377-379"""


def _refuse(what: str):
    raise ValueError(f"dc_ae: {what} is not built on the HIP path (csrc/dc_ae.hip serves the video decoder and encoder of "
                     "dc-ae-f32t4c128: rms3d norms, silu / relu, InterpolateConv upsampling, strided Conv downsampling, "
                     "duplicating / averaging shortcuts, ResBlock and EViTS5_GLU blocks)")


def _pow2_8(c: int) -> bool:
    return c >= 8 and c & (c - 1) == 0


class ConvLayer(_Holder):
    """ops.py:56-136 with is_video=True: `.conv` (the padding is F.pad's, so the Conv3d itself has none) and `.norm`"""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int = 3, groups: int = 1, use_bias: bool = False,
                 norm: Optional[str] = None, act_func: Optional[str] = None, stride=1):
        super().__init__()
        self.stride = (stride,) * 3 if isinstance(stride, int) else tuple(stride)
        if norm not in (None, "rms3d"):
            _refuse(f"norm {norm!r}")
        if act_func not in (None, "silu"):
            _refuse(f"activation {act_func!r}")
        self.conv = nn.Conv3d(in_channels, out_channels, kernel_size, stride=self.stride, groups=groups, bias=use_bias)
        self.norm = RMSNorm3d(out_channels) if norm == "rms3d" else None
        self.act = act_func


class InterpolateConvUpSampleLayer(_Holder):
    """ops.py:260-295"""

    def __init__(self, in_channels: int, out_channels: int, temporal_upsample: bool):
        super().__init__()
        self.factor, self.mode, self.temporal_upsample = 2, "nearest", temporal_upsample
        self.conv = ConvLayer(in_channels, out_channels, 3, use_bias=True)


class ChannelDuplicatingPixelShuffleUpSampleLayer(_Holder):
    """ops.py:301-337"""

    def __init__(self, in_channels: int, out_channels: int, factor: int, temporal_upsample: bool = False):
        super().__init__()
        assert out_channels * factor ** 2 % in_channels == 0
        self.in_channels, self.out_channels, self.factor, self.temporal_upsample = in_channels, out_channels, factor, temporal_upsample


class PixelUnshuffleChannelAveragingDownSampleLayer(_Holder):
    """ops.py:189-228 (no parameters)"""

    def __init__(self, in_channels: int, out_channels: int, factor: int, temporal_downsample: bool = False):
        super().__init__()
        self.in_channels, self.out_channels, self.factor, self.temporal_downsample = in_channels, out_channels, factor, temporal_downsample


class ResBlock(_Holder):
    """ops.py:594-639 as build_block builds it (dc_ae.py:119-131)"""

    def __init__(self, channels: int, norm: str, act: str):
        super().__init__()
        self.conv1 = ConvLayer(channels, channels, 3, use_bias=True, act_func=act)
        self.conv2 = ConvLayer(channels, channels, 3, use_bias=False, norm=norm)


class GLUMBConv(_Holder):
    """ops.py:530-591 as EfficientViTBlock builds it (:870-881): expand_ratio 4, bias (True, True, False)"""

    def __init__(self, channels: int, norm: str, act: str):
        super().__init__()
        mid = 4 * channels
        self.inverted_conv = ConvLayer(channels, 2 * mid, 1, use_bias=True, act_func=act)
        self.depth_conv = ConvLayer(2 * mid, 2 * mid, 3, groups=2 * mid, use_bias=True)
        self.point_conv = ConvLayer(mid, channels, 1, use_bias=False, norm=norm)


class LiteMLA(_Holder):
    """ops.py:642-823 as EfficientViTBlock builds it (:842-853): dim 32, scales (5,), no bias, relu kernel"""

    def __init__(self, channels: int, norm: str, scales: tuple = (5,), dim: int = 32):
        super().__init__()
        heads = channels // dim
        total = heads * dim
        self.dim, self.eps = dim, 1.0e-15
        self.qkv = ConvLayer(channels, 3 * total, 1)
        self.aggreg = nn.ModuleList([
            nn.Sequential(nn.Conv3d(3 * total, 3 * total, s, padding=s // 2, groups=3 * total, bias=False),
                          nn.Conv3d(3 * total, 3 * total, 1, groups=3 * heads, bias=False)) for s in scales])
        self.proj = ConvLayer(total * (1 + len(scales)), channels, 1, norm=norm)


class ResidualBlock(_Holder):
    """ops.py:896-926"""

    def __init__(self, main: nn.Module, shortcut: Optional[nn.Module]):
        super().__init__()
        self.pre_norm = None
        self.main = main
        self.shortcut = shortcut
        self.post_act = None


class EfficientViTBlock(_Holder):
    """ops.py:826-888"""

    def __init__(self, channels: int, norm: str, act: str, scales: tuple = (5,)):
        super().__init__()
        self.context_module = ResidualBlock(LiteMLA(channels, norm, scales), IdentityLayer())
        self.local_module = ResidualBlock(GLUMBConv(channels, norm, act), IdentityLayer())


class OpSequential(_Holder):
    """ops.py:966-978"""

    def __init__(self, op_list: list):
        super().__init__()
        self.op_list = nn.ModuleList([op for op in op_list if op is not None])


class _ReLU(_Holder):
    """the parameter-free nn.ReLU slot of project_out (keeps its conv at op_list.2)"""


def _per_stage(v, stage_id: int):
    return v[stage_id] if isinstance(v, (list, tuple)) else v


def _build_block(bt: str, width: int, nm: str, ac: str) -> nn.Module:
    """build_block (dc_ae.py:119-143) for the two block types the kernels serve"""
    return ResidualBlock(ResBlock(width, nm, ac), IdentityLayer()) if bt == "ResBlock" else EfficientViTBlock(width, nm, ac, scales=(5,))


class Encoder(_Holder):
    """dc_ae.py:376-440.  Refuses, at construction, what the kernels cannot take."""

    def __init__(self, cfg: EncoderConfig):
        super().__init__()
        self.cfg = cfg
        n = len(cfg.width_list)
        self.num_stages = n
        assert len(cfg.depth_list) == n
        assert isinstance(cfg.block_type, str) or (isinstance(cfg.block_type, (list, tuple)) and len(cfg.block_type) == n)
        if not cfg.is_video:
            _refuse("the 2-D image encoder (is_video=False)")
        if cfg.downsample_block_type != "Conv":
            _refuse(f"downsample_block_type {cfg.downsample_block_type!r}")
        if cfg.downsample_shortcut != "averaging" or cfg.out_shortcut != "averaging":
            _refuse(f"shortcuts {cfg.downsample_shortcut!r} / {cfg.out_shortcut!r}")
        if cfg.out_norm is not None or cfg.out_act is not None:
            _refuse(f"encoder project_out norm / act {cfg.out_norm!r} / {cfg.out_act!r}")
        if cfg.double_latent:
            _refuse("double_latent=True")
        if not cfg.downsample_match_channel:
            _refuse("downsample_match_channel=False")
        if cfg.depth_list[0] <= 0:
            _refuse("depth_list[0] == 0 (a downsampling project_in)")
        if cfg.in_channels > 8 and not _pow2_8(cfg.in_channels):
            _refuse(f"in_channels {cfg.in_channels} (osk_conv3d_zp_ndhwc_bf16 takes Cin = 8 * 2^j; up to 8 are zero-padded to 8)")
        for stage_id, width in enumerate(cfg.width_list):
            bt, nm, ac = (_per_stage(v, stage_id) for v in (cfg.block_type, cfg.norm, cfg.act))
            if cfg.depth_list[stage_id] <= 0 and stage_id != n - 1:
                _refuse(f"an empty stage {stage_id}")
            if bt not in ("ResBlock", "EViTS5_GLU"):
                _refuse(f"block_type {bt!r}")
            if nm != "rms3d":
                _refuse(f"norm {nm!r}")
            if ac != "silu":
                _refuse(f"activation {ac!r}")
            if not _pow2_8(width) or width < 32:
                _refuse(f"width {width} (conv / attention kernels take 8 * 2^j >= 32 channels)")
        if cfg.latent_channels % 8 or cfg.width_list[-1] % cfg.latent_channels:
            _refuse(f"latent_channels {cfg.latent_channels} against width {cfg.width_list[-1]} (the averaging shortcut)")
        temporal = tuple(cfg.temporal_downsample) if cfg.temporal_downsample else (False,) * n

        self.project_in = ConvLayer(cfg.in_channels, cfg.width_list[0], 3, use_bias=True)
        stages: list = []
        for stage_id, (width, depth) in enumerate(zip(cfg.width_list, cfg.depth_list)):
            bt, nm, ac = (_per_stage(v, stage_id) for v in (cfg.block_type, cfg.norm, cfg.act))
            stage: list = [_build_block(bt, width, nm, ac) for _ in range(depth)]
            if stage_id < n - 1 and depth > 0:
                cout = cfg.width_list[stage_id + 1]
                per = 8 if temporal[stage_id] else 4
                if width * per % cout or width * 4 % cout:    # the T == 1 branch averages over the 2-D groups
                    _refuse(f"downsample {width} -> {cout} (the averaging shortcut needs in * {per} % out == 0)")
                stage.append(ResidualBlock(
                    ConvLayer(width, cout, 3, use_bias=True, stride=(2 if temporal[stage_id] else 1, 2, 2)),
                    PixelUnshuffleChannelAveragingDownSampleLayer(width, cout, factor=2, temporal_downsample=temporal[stage_id])))
            stages.append(OpSequential(stage))
        self.stages = nn.ModuleList(stages)
        self.project_out = ResidualBlock(
            OpSequential([None, None, ConvLayer(cfg.width_list[-1], cfg.latent_channels, 3, use_bias=True)]),
            PixelUnshuffleChannelAveragingDownSampleLayer(cfg.width_list[-1], cfg.latent_channels, factor=1))


class Decoder(_Holder):
    """dc_ae.py:443-519.  Refuses, at construction, what the kernels cannot take."""

    def __init__(self, cfg: DecoderConfig):
        super().__init__()
        self.cfg = cfg
        n = len(cfg.width_list)
        self.num_stages = n
        assert len(cfg.depth_list) == n
        assert isinstance(cfg.block_type, str) or (isinstance(cfg.block_type, (list, tuple)) and len(cfg.block_type) == n)
        if not cfg.is_video:
            _refuse("the 2-D image decoder (is_video=False)")
        if cfg.upsample_block_type != "InterpolateConv":
            _refuse(f"upsample_block_type {cfg.upsample_block_type!r}")
        if cfg.in_shortcut != "duplicating" or cfg.upsample_shortcut != "duplicating":
            _refuse(f"shortcuts {cfg.in_shortcut!r} / {cfg.upsample_shortcut!r}")
        if not cfg.upsample_match_channel:
            _refuse("upsample_match_channel=False")
        if cfg.out_norm != "rms3d" or cfg.out_act != "relu":
            _refuse(f"project_out norm / act {cfg.out_norm!r} / {cfg.out_act!r}")
        if cfg.depth_list[0] <= 0:
            _refuse("depth_list[0] == 0 (an upsampling project_out)")
        if not _pow2_8(cfg.latent_channels):
            _refuse(f"latent_channels {cfg.latent_channels} (osk_conv3d_zp_ndhwc_bf16 takes Cin = 8 * 2^j)")
        if cfg.latent_channels > cfg.width_list[-1] or cfg.width_list[-1] % cfg.latent_channels:
            _refuse(f"latent_channels {cfg.latent_channels} against width {cfg.width_list[-1]} (the duplicating shortcut)")
        for stage_id, width in enumerate(cfg.width_list):
            bt, nm, ac = (_per_stage(v, stage_id) for v in (cfg.block_type, cfg.norm, cfg.act))
            if cfg.depth_list[stage_id] <= 0 and stage_id != n - 1:
                _refuse(f"an empty stage {stage_id}")
            if bt not in ("ResBlock", "EViTS5_GLU"):
                _refuse(f"block_type {bt!r}")
            if nm != "rms3d":
                _refuse(f"norm {nm!r}")
            if ac != "silu":
                _refuse(f"activation {ac!r}")
            if not _pow2_8(width) or width < 32:
                _refuse(f"width {width} (conv / attention kernels take 8 * 2^j >= 32 channels)")
        temporal = tuple(cfg.temporal_upsample) if cfg.temporal_upsample else (False,) * n

        self.project_in = ResidualBlock(
            ConvLayer(cfg.latent_channels, cfg.width_list[-1], 3, use_bias=True),
            ChannelDuplicatingPixelShuffleUpSampleLayer(cfg.latent_channels, cfg.width_list[-1], factor=1))
        stages: list = []
        for stage_id, (width, depth) in reversed(list(enumerate(zip(cfg.width_list, cfg.depth_list)))):
            stage: list = []
            if stage_id < n - 1 and depth > 0:
                cin = cfg.width_list[stage_id + 1]
                if width * 4 % cin:
                    _refuse(f"upsample {cin} -> {width} (the duplicating shortcut needs 4 * out % in == 0)")
                stage.append(ResidualBlock(
                    InterpolateConvUpSampleLayer(cin, width, temporal[stage_id]),
                    ChannelDuplicatingPixelShuffleUpSampleLayer(cin, width, factor=2, temporal_upsample=temporal[stage_id])))
            bt, nm, ac = (_per_stage(v, stage_id) for v in (cfg.block_type, cfg.norm, cfg.act))
            for _ in range(depth):
                stage.append(_build_block(bt, width, nm, ac))
            stages.insert(0, OpSequential(stage))
        self.stages = nn.ModuleList(stages)
        self.project_out = OpSequential([RMSNorm3d(cfg.width_list[0]), _ReLU(),
                                         ConvLayer(cfg.width_list[0], cfg.in_channels, 3, use_bias=True)])
        self.disc_off_grad_ckpt = False


# =============================================================================================
# engine: kernels over NDHWC tensors
# =============================================================================================
class _DensePlan:
    """Conv3d weight [Cout, Cin, k, k, k] -> bf16 [Cout, round_up(k^3 * Cin, 64)], K = tap-major / channel-minor; bias f32.
    cin_pad: Cin below it is widened to it with zero columns (the encoder's 3-channel project_in runs as an 8-channel conv)"""

    def __init__(self, conv: nn.Conv3d, cin_pad: int = 0):
        w = conv.weight.detach()
        co, ci, k = w.shape[0], w.shape[1], w.shape[2]
        if ci < cin_pad:
            w = torch.nn.functional.pad(w.permute(0, 2, 3, 4, 1), (0, cin_pad - ci)).permute(0, 4, 1, 2, 3)
            ci = cin_pad
        K = k ** 3 * ci
        Kp = (K + 63) // 64 * 64
        self.w = torch.zeros(co, Kp, dtype=BF16, device=w.device)
        self.w[:, :K] = w.permute(0, 2, 3, 4, 1).reshape(co, K).to(BF16)
        self.b = None if conv.bias is None else conv.bias.detach().float().contiguous()
        self.cin, self.cout, self.k = ci, co, k


class _DepthwisePlan:
    """depthwise Conv3d weight [C, 1, k, k, k] -> bf16 [k^3, C]; bias f32"""

    def __init__(self, conv: nn.Conv3d):
        w = conv.weight.detach()
        C, k = w.shape[0], w.shape[2]
        self.w = w.reshape(C, k ** 3).t().contiguous().to(BF16)
        self.b = None if conv.bias is None else conv.bias.detach().float().contiguous()
        self.k = k


def _plan(mod: nn.Module, kind: str):
    """kernel-side image of a layer's parameters, cached on the layer and keyed on the parameters' (storage pointer, in-place
    version); DCAE.load_state_dict / invalidate_plan drop every cache."""
    key = tuple((q.data_ptr(), 0 if q.is_inference() else q._version) for q in mod.parameters())
    c = mod.__dict__.get("_osk_plan")
    if c is not None and c[0] == key:
        return c[1]
    if kind == "dense":
        p = _DensePlan(mod)
    elif kind == "dense_pad8":
        p = _DensePlan(mod, cin_pad=8)
    elif kind == "depthwise":
        p = _DepthwisePlan(mod)
    elif kind == "group32":
        p = mod.weight.detach().reshape(mod.weight.shape[0], 32).to(BF16).contiguous()
    else:  # "norm"
        p = (mod.weight.detach().float().contiguous(), mod.bias.detach().float().contiguous())
    mod.__dict__["_osk_plan"] = (key, p)
    return p


def _conv(layer: ConvLayer, x: Tensor, up_t: bool = False, up_hw: bool = False, res: Tensor | None = None,
          kind: str = "dense") -> Tensor:
    """ConvLayer.forward without its norm: zero padding, conv, bias, act (+ upsample in front, + shortcut add behind)"""
    p = _plan(layer.conv, kind)
    B, T, H, W, C = x.shape
    assert C == p.cin, (C, p.cin)
    out = torch.empty(B, T << int(up_t), H << int(up_hw), W << int(up_hw), p.cout, dtype=BF16, device=x.device)
    return _ops().conv3d_zp(x, p.w, p.b, out, p.k, up_t, up_hw, layer.act == "silu", res)


def _pointwise(layer: ConvLayer, x: Tensor) -> Tensor:
    """a 1x1x1 ConvLayer without its norm: a row GEMM (osk_gemm_bf16) where its K % 64 rule allows and no SiLU follows, else
    the k = 1 form of the conv kernel"""
    p = _plan(layer.conv, "dense")
    if layer.act is None and p.cin % 64 == 0:
        B, T, H, W, C = x.shape
        out = torch.empty(B, T, H, W, p.cout, dtype=BF16, device=x.device)
        _ops().gemm(x.view(1, -1, C), p.w, p.b, out.view(1, -1, p.cout))
        return out
    return _conv(layer, x)


def _rms(norm: RMSNorm3d, x: Tensor, res: Tensor | None = None, relu: bool = False) -> Tensor:
    w, b = _plan(norm, "norm")
    return _ops().rmsnorm_affine(x, w, b, torch.empty_like(x), norm.eps, res, relu)


def _shortcut(sc: ChannelDuplicatingPixelShuffleUpSampleLayer, x: Tensor, temporal: bool) -> Tensor:
    B, T, H, W, _ = x.shape
    ft, fhw = (2 if temporal else 1), sc.factor
    out = torch.empty(B, T * ft, H * fhw, W * fhw, sc.out_channels, dtype=BF16, device=x.device)
    return _ops().dup_shuffle(x, out, ft, fhw)


def _upsample(blk: ResidualBlock, x: Tensor) -> Tensor:
    """ResidualBlock(InterpolateConvUpSampleLayer, ChannelDuplicatingPixelShuffleUpSampleLayer): both take the 2-D branch for
    a single frame (ops.py:290, 321)"""
    temporal = bool(blk.main.temporal_upsample) and x.shape[1] != 1
    return _conv(blk.main.conv, x, up_t=temporal, up_hw=True, res=_shortcut(blk.shortcut, x, temporal))


def _res_block(blk: ResidualBlock, x: Tensor) -> Tensor:
    """x + rms(conv2(silu(conv1(x))))"""
    m = blk.main
    return _rms(m.conv2.norm, _conv(m.conv2, _conv(m.conv1, x)), res=x)


def _lite_mla(blk: ResidualBlock, x: Tensor) -> Tensor:
    """x + LiteMLA(x) (ops.py:800-823)"""
    m = blk.main
    B, T, H, W, C = x.shape
    N = T * H * W
    scales = [_pointwise(m.qkv, x)]
    for agg in m.aggreg:
        dw = _plan(agg[0], "depthwise")
        t = _ops().dwconv3d(scales[0], dw.w, dw.b, torch.empty_like(scales[0]), dw.k)
        scales.append(_ops().gconv32(t, _plan(agg[1], "group32"), torch.empty_like(t)))
    att = torch.empty(B, T, H, W, C * len(scales), dtype=BF16, device=x.device)
    for i, s in enumerate(scales):
        _ops().relu_linear_attn(s.view(B, N, 3 * C), att.view(B, N, -1)[:, :, i * C:], m.eps)
    return _rms(m.proj.norm, _pointwise(m.proj, att), res=x)


def _glu_mbconv(blk: ResidualBlock, x: Tensor) -> Tensor:
    """x + GLUMBConv(x) (ops.py:582-591)"""
    m = blk.main
    h = _pointwise(m.inverted_conv, x)
    dw = _plan(m.depth_conv.conv, "depthwise")
    B, T, H, W, C2 = h.shape
    g = _ops().dwconv3d(h, dw.w, dw.b, torch.empty(B, T, H, W, C2 // 2, dtype=BF16, device=x.device), dw.k, glu=True)
    return _rms(m.point_conv.norm, _pointwise(m.point_conv, g), res=x)


def run_decoder(dec: Decoder, z: Tensor) -> Tensor:
    """Decoder.forward (dc_ae.py:507-519) on an NDHWC bf16 latent -> NDHWC bf16 video"""
    pi = dec.project_in
    x = _conv(pi.main, z, res=_shortcut(pi.shortcut, z, False))
    for stage in reversed(dec.stages):
        for op in stage.op_list:
            if isinstance(op, EfficientViTBlock):
                x = _glu_mbconv(op.local_module, _lite_mla(op.context_module, x))
            elif isinstance(op.main, ResBlock):
                x = _res_block(op, x)
            else:
                x = _upsample(op, x)
    po = dec.project_out.op_list
    return _conv(po[2], _rms(po[0], x, relu=True))


def _avg_shortcut(sc: PixelUnshuffleChannelAveragingDownSampleLayer, x: Tensor, temporal: bool) -> Tensor:
    B, T, H, W, _ = x.shape
    ft, fhw = (2 if temporal else 1), sc.factor
    out = torch.empty(B, T // ft, H // fhw, W // fhw, sc.out_channels, dtype=BF16, device=x.device)
    return _ops().unshuffle_avg(x, out, ft, fhw)


def _downsample(blk: ResidualBlock, x: Tensor) -> Tensor:
    """ResidualBlock(ConvLayer(stride), PixelUnshuffleChannelAveragingDownSampleLayer): the shortcut takes its 2-D branch for a
    single frame (ops.py:213); the conv's temporal stride is the configured one whatever T is"""
    layer = blk.main
    p = _plan(layer.conv, "dense")
    B, T, H, W, C = x.shape
    assert C == p.cin, (C, p.cin)
    st = layer.stride[0]
    res = _avg_shortcut(blk.shortcut, x, bool(blk.shortcut.temporal_downsample) and T != 1)
    out = torch.empty(B, (T - 1) // st + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1, p.cout, dtype=BF16, device=x.device)
    return _ops().conv3d_zp_strided(x, p.w, p.b, out, st, res)


def run_encoder(enc: Encoder, x: Tensor) -> Tensor:
    """Encoder.forward (dc_ae.py:431-440) on an NDHWC bf16 video whose channels are zero-padded to 8 -> NDHWC bf16 latent"""
    x = _conv(enc.project_in, x, kind="dense_pad8")
    for stage in enc.stages:
        for op in stage.op_list:
            if isinstance(op, EfficientViTBlock):
                x = _glu_mbconv(op.local_module, _lite_mla(op.context_module, x))
            elif isinstance(op.main, ResBlock):
                x = _res_block(op, x)
            else:
                x = _downsample(op, x)
    po = enc.project_out
    return _conv(po.main.op_list[0], x, res=_avg_shortcut(po.shortcut, x, False))


# =============================================================================================
# the model
# =============================================================================================
class DCAE(nn.Module):
    """dc_ae.py:522-787; the encoder half only with cfg.build_encoder"""

    def __init__(self, cfg: DCAEConfig):
        super().__init__()
        self.cfg = cfg
        if cfg.use_quant_conv:
            _refuse("use_quant_conv")
        if cfg.build_encoder:
            self.encoder = Encoder(cfg.encoder)
        self.decoder = Decoder(cfg.decoder)
        self.scaling_factor = cfg.scaling_factor
        self.time_compression_ratio = cfg.time_compression_ratio
        self.spatial_compression_ratio = cfg.spatial_compression_ratio
        self.use_spatial_tiling = cfg.use_spatial_tiling
        self.use_temporal_tiling = cfg.use_temporal_tiling
        self.spatial_tile_size = cfg.spatial_tile_size
        self.temporal_tile_size = cfg.temporal_tile_size
        assert cfg.spatial_tile_size // cfg.spatial_compression_ratio
        self.spatial_tile_latent_size = cfg.spatial_tile_size // cfg.spatial_compression_ratio
        assert cfg.temporal_tile_size // cfg.time_compression_ratio
        self.temporal_tile_latent_size = cfg.temporal_tile_size // cfg.time_compression_ratio
        self.tile_overlap_factor = cfg.tile_overlap_factor
        if cfg.pretrained_path is not None:
            self.load_model()

    def load_model(self):
        if self.cfg.pretrained_source != "dc-ae":
            raise NotImplementedError
        self.load_state_dict(torch.load(self.cfg.pretrained_path, map_location="cpu", weights_only=True)["state_dict"])

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """Without cfg.build_encoder the `encoder.*` entries of a full reference checkpoint are DROPPED here -- the module then
        builds the decoder only.  Every remaining key is loaded as nn.Module.load_state_dict would (strict by default)."""
        kept = state_dict if self.cfg.build_encoder else {k: v for k, v in state_dict.items() if not k.startswith("encoder.")}
        self.invalidate_plan()
        return super().load_state_dict(kept, strict=strict, assign=assign)

    def invalidate_plan(self):
        for m in self.modules():
            m.__dict__.pop("_osk_plan", None)

    def get_last_layer(self):
        return self.decoder.project_out.op_list[2].conv.weight

    def _need_encoder(self):
        if not self.cfg.build_encoder:
            raise NotImplementedError("dc_ae: this model holds only the DC-AE DECODER (inference needs decode alone), so "
                                      "DCAE.encode / forward cannot run; build it with DCAEConfig(build_encoder=True) or "
                                      "DC_AE_with_encoder(...) to get the encoder (dc_ae.py:376-440) as well")

    def _check_encode_shape(self, x: Tensor):
        """what the reference meets as an assert inside pixel_unshuffle_3d (vo_ops.py:45-47), here before anything is launched"""
        if x.dim() != 5:
            raise ValueError(f"dc_ae: encode takes [B, C, T, H, W], got shape {tuple(x.shape)}")
        _, C, T, H, W = x.shape
        r = self.spatial_compression_ratio
        if C != self.encoder.cfg.in_channels:
            raise ValueError(f"dc_ae: encode takes {self.encoder.cfg.in_channels} channels, got shape {tuple(x.shape)}")
        if H % r or W % r:
            raise ValueError(f"dc_ae: cannot encode shape {tuple(x.shape)}: H and W must be multiples of {r}")
        cfg = self.encoder.cfg
        t = T
        for stage_id in range(self.encoder.num_stages - 1):
            if cfg.temporal_downsample and cfg.temporal_downsample[stage_id] and cfg.depth_list[stage_id] > 0 and t != 1:
                if t % 2:
                    raise ValueError(f"dc_ae: cannot encode shape {tuple(x.shape)}: T must be 1 or even at every temporal "
                                     f"downsample (it is {t} at stage {stage_id})")
                t //= 2

    def encode_single(self, x: Tensor, is_video_encoder: bool = True) -> Tensor:
        """dc_ae.py:564-578 for the video encoder: ONE NCTHW -> NDHWC conversion in (channels zero-padded to 8), one out"""
        assert x.shape[0] == 1 and x.dim() == 5 and is_video_encoder
        _, C, T, H, W = x.shape
        xl = torch.zeros(1, T, H, W, max(C, 8), dtype=BF16, device=x.device)
        xl[..., :C].copy_(x.permute(0, 2, 3, 4, 1))
        z = run_encoder(self.encoder, xl).permute(0, 4, 1, 2, 3).contiguous().to(x.dtype)
        if self.scaling_factor is not None:
            z = z / self.scaling_factor
        return z

    def _encode(self, x: Tensor) -> Tensor:
        self._need_encoder()
        if self.cfg.is_training:
            _refuse("is_training=True")
        self._check_encode_shape(x)
        return torch.cat([self.encode_single(x[i: i + 1], True) for i in range(x.shape[0])], dim=0)

    def spatial_tiled_encode(self, x: Tensor) -> Tensor:
        net_size = int(self.spatial_tile_size * (1 - self.tile_overlap_factor))
        blend_extent = int(self.spatial_tile_latent_size * self.tile_overlap_factor)
        row_limit = self.spatial_tile_latent_size - blend_extent
        rows = []
        for i in range(0, x.shape[-2], net_size):
            row = []
            for j in range(0, x.shape[-1], net_size):
                tile = x[:, :, :, i: i + self.spatial_tile_size, j: j + self.spatial_tile_size]
                row.append(self._encode(tile))
            rows.append(row)
        result_rows = []
        for i, row in enumerate(rows):
            result_row = []
            for j, tile in enumerate(row):
                if i > 0:
                    tile = self.blend_v(rows[i - 1][j], tile, blend_extent)
                if j > 0:
                    tile = self.blend_h(row[j - 1], tile, blend_extent)
                result_row.append(tile[:, :, :, :row_limit, :row_limit])
            result_rows.append(torch.cat(result_row, dim=-1))
        return torch.cat(result_rows, dim=-2)

    def temporal_tiled_encode(self, x: Tensor) -> Tensor:
        overlap_size = int(self.temporal_tile_size * (1 - self.tile_overlap_factor))
        blend_extent = int(self.temporal_tile_latent_size * self.tile_overlap_factor)
        t_limit = self.temporal_tile_latent_size - blend_extent
        row = []
        for i in range(0, x.shape[2], overlap_size):
            tile = x[:, :, i: i + self.temporal_tile_size, :, :]
            if self.use_spatial_tiling and (tile.shape[-1] > self.spatial_tile_size or tile.shape[-2] > self.spatial_tile_size):
                tile = self.spatial_tiled_encode(tile)
            else:
                tile = self._encode(tile)
            row.append(tile)
        result_row = []
        for i, tile in enumerate(row):
            if i > 0:
                tile = self.blend_t(row[i - 1], tile, blend_extent)
            result_row.append(tile[:, :, :t_limit, :, :])
        return torch.cat(result_row, dim=2)

    def encode(self, x: Tensor) -> Tensor:
        self._need_encoder()
        if self.use_temporal_tiling and x.shape[2] > self.temporal_tile_size:
            return self.temporal_tiled_encode(x)
        elif self.use_spatial_tiling and (x.shape[-1] > self.spatial_tile_size or x.shape[-2] > self.spatial_tile_size):
            return self.spatial_tiled_encode(x)
        else:
            return self._encode(x)

    def forward(self, x: Tensor):
        """dc_ae.py:761-778 -> (dec, None, z)"""
        self._need_encoder()
        x_type = x.dtype
        is_image_model = self.cfg.__dict__.get("is_image_model", False)
        x = x.to(self.encoder.project_in.conv.weight.dtype)
        if is_image_model:
            b, c, _, h, w = x.shape
            x = x.permute(0, 2, 1, 3, 4).reshape(-1, c, h, w)
        z = self.encode(x)
        dec = self.decode(z)
        if is_image_model:
            dec = dec.reshape(b, 1, c, h, w).permute(0, 2, 1, 3, 4)
            z = z.unsqueeze(dim=0).permute(0, 2, 1, 3, 4)
        dec = dec.to(x_type)
        return dec, None, z

    # ---- tiling (dc_ae.py:589-611, 613-672, 674-725): the reference's loops; a cross-fade is ONE launch of osk_blend_bf16
    @staticmethod
    def _blend(a: Tensor, b: Tensor, extent: int, dim: int) -> Tensor:
        if b.dtype == BF16 and a.dtype == BF16 and a.is_contiguous() and b.is_contiguous():
            return _ops().blend(a, b, extent, dim)
        bb = b.to(BF16).contiguous()
        _ops().blend(a.to(BF16).contiguous(), bb, extent, dim)
        b.copy_(bb)
        return b

    def blend_v(self, a: Tensor, b: Tensor, blend_extent: int) -> Tensor:
        return self._blend(a, b, blend_extent, -2)

    def blend_h(self, a: Tensor, b: Tensor, blend_extent: int) -> Tensor:
        return self._blend(a, b, blend_extent, -1)

    def blend_t(self, a: Tensor, b: Tensor, blend_extent: int) -> Tensor:
        return self._blend(a, b, blend_extent, -3)

    def spatial_tiled_decode(self, z: Tensor) -> Tensor:
        net_size = int(self.spatial_tile_latent_size * (1 - self.tile_overlap_factor))
        blend_extent = int(self.spatial_tile_size * self.tile_overlap_factor)
        row_limit = self.spatial_tile_size - blend_extent
        rows = []
        for i in range(0, z.shape[-2], net_size):
            row = []
            for j in range(0, z.shape[-1], net_size):
                tile = z[:, :, :, i: i + self.spatial_tile_latent_size, j: j + self.spatial_tile_latent_size]
                row.append(self._decode(tile))
            rows.append(row)
        result_rows = []
        for i, row in enumerate(rows):
            result_row = []
            for j, tile in enumerate(row):
                if i > 0:
                    tile = self.blend_v(rows[i - 1][j], tile, blend_extent)
                if j > 0:
                    tile = self.blend_h(row[j - 1], tile, blend_extent)
                result_row.append(tile[:, :, :, :row_limit, :row_limit])
            result_rows.append(torch.cat(result_row, dim=-1))
        return torch.cat(result_rows, dim=-2)

    def temporal_tiled_decode(self, z: Tensor) -> Tensor:
        overlap_size = int(self.temporal_tile_latent_size * (1 - self.tile_overlap_factor))
        blend_extent = int(self.temporal_tile_size * self.tile_overlap_factor)
        t_limit = self.temporal_tile_size - blend_extent
        row = []
        for i in range(0, z.shape[2], overlap_size):
            tile = z[:, :, i: i + self.temporal_tile_latent_size, :, :]
            if self.use_spatial_tiling and (
                tile.shape[-1] > self.spatial_tile_latent_size or tile.shape[-2] > self.spatial_tile_latent_size
            ):
                decoded = self.spatial_tiled_decode(tile)
            else:
                decoded = self._decode(tile)
            row.append(decoded)
        result_row = []
        for i, tile in enumerate(row):
            if i > 0:
                tile = self.blend_t(row[i - 1], tile, blend_extent)
            result_row.append(tile[:, :, :t_limit, :, :])
        return torch.cat(result_row, dim=2)

    def decode_single(self, z: Tensor, is_video_decoder: bool = True) -> Tensor:
        """dc_ae.py:727-740 for the video decoder: ONE NCTHW -> NDHWC conversion in, one out"""
        assert z.shape[0] == 1 and z.dim() == 5 and is_video_decoder
        if self.scaling_factor is not None:
            z = z * self.scaling_factor
        zl = z.permute(0, 2, 3, 4, 1).to(BF16).contiguous()
        x = run_decoder(self.decoder, zl)
        return x.permute(0, 4, 1, 2, 3).contiguous().to(z.dtype)

    def _decode(self, z: Tensor) -> Tensor:
        if self.cfg.is_training:
            _refuse("is_training=True")
        return torch.cat([self.decode_single(z[i: i + 1], True) for i in range(z.shape[0])], dim=0)

    def decode(self, z: Tensor) -> Tensor:
        if self.use_temporal_tiling and z.shape[2] > self.temporal_tile_latent_size:
            return self.temporal_tiled_decode(z)
        elif self.use_spatial_tiling and (
            z.shape[-1] > self.spatial_tile_latent_size or z.shape[-2] > self.spatial_tile_latent_size
        ):
            return self.spatial_tiled_decode(z)
        else:
            return self._decode(z)

    def get_latent_size(self, input_size: list) -> list:
        latent_size = [(input_size[0] - 1) // self.time_compression_ratio + 1]
        for i in range(1, 3):
            latent_size.append((input_size[i] - 1) // self.spatial_compression_ratio + 1)
        return latent_size


REGISTERED_DCAE_MODEL = {"dc-ae-f32t4c128": (dc_ae_f32, None)}


def create_dc_ae_model_cfg(name: str, pretrained_path: Optional[str] = None) -> DCAEConfig:
    """ae_model_zoo.py:37-42"""
    assert name in REGISTERED_DCAE_MODEL, f"{name} is not supported"
    fn, default_path = REGISTERED_DCAE_MODEL[name]
    return fn(name, default_path if pretrained_path is None else pretrained_path)


def _build_dc_ae(build_encoder: bool, model_name, device_map, torch_dtype, from_scratch, from_pretrained, is_training,
                 use_spatial_tiling, use_temporal_tiling, spatial_tile_size, temporal_tile_size, tile_overlap_factor, scaling_factor,
                 disc_off_grad_ckpt) -> DCAE:
    if is_training:
        _refuse("is_training=True")
    if not from_scratch and from_pretrained is None:
        raise ValueError("dc_ae: from_scratch=False needs from_pretrained=<local checkpoint> (no hub download on this path)")
    cfg = create_dc_ae_model_cfg(model_name)
    cfg.build_encoder = build_encoder
    with torch.device(device_map):
        model = DCAE(cfg).to(torch_dtype)
    if from_pretrained is not None:
        from .ckpt import load_checkpoint
        model = load_checkpoint(model, from_pretrained, device_map=device_map)
    model.cfg.is_training = is_training
    model.use_spatial_tiling = use_spatial_tiling
    model.use_temporal_tiling = use_temporal_tiling
    model.spatial_tile_size = spatial_tile_size
    model.temporal_tile_size = temporal_tile_size
    model.tile_overlap_factor = tile_overlap_factor
    if scaling_factor is not None:
        model.scaling_factor = scaling_factor
    model.decoder.disc_off_grad_ckpt = disc_off_grad_ckpt
    return model


def DC_AE(
    model_name: str,
    device_map: str | torch.device = "cuda",
    torch_dtype: torch.dtype = torch.bfloat16,
    from_scratch: bool = False,
    from_pretrained: str | None = None,
    is_training: bool = False,
    use_spatial_tiling: bool = False,
    use_temporal_tiling: bool = False,
    spatial_tile_size: int = 256,
    temporal_tile_size: int = 32,
    tile_overlap_factor: float = 0.25,
    scaling_factor: float = None,
    disc_off_grad_ckpt: bool = False,
) -> DCAE:
    """ae_model_zoo.py:52-85 (registered there as "dc_ae").  The reference's `from_scratch=False` pulls the weights from the
    Hugging Face hub by model name; this package loads local files only: pass `from_pretrained=<checkpoint>` (a full
    checkpoint's encoder.* keys are dropped, see DCAE.load_state_dict) or `from_scratch=True`."""
    return _build_dc_ae(False, model_name, device_map, torch_dtype, from_scratch, from_pretrained, is_training, use_spatial_tiling,
                        use_temporal_tiling, spatial_tile_size, temporal_tile_size, tile_overlap_factor, scaling_factor,
                        disc_off_grad_ckpt)


def DC_AE_with_encoder(
    model_name: str,
    device_map: str | torch.device = "cuda",
    torch_dtype: torch.dtype = torch.bfloat16,
    from_scratch: bool = False,
    from_pretrained: str | None = None,
    is_training: bool = False,
    use_spatial_tiling: bool = False,
    use_temporal_tiling: bool = False,
    spatial_tile_size: int = 256,
    temporal_tile_size: int = 32,
    tile_overlap_factor: float = 0.25,
    scaling_factor: float = None,
    disc_off_grad_ckpt: bool = False,
) -> DCAE:
    """DC_AE with the encoder half built as well (DCAEConfig.build_encoder): `encode` and `forward` run, and a checkpoint's
    encoder.* keys are loaded strictly instead of dropped."""
    return _build_dc_ae(True, model_name, device_map, torch_dtype, from_scratch, from_pretrained, is_training, use_spatial_tiling,
                        use_temporal_tiling, spatial_tile_size, temporal_tile_size, tile_overlap_factor, scaling_factor,
                        disc_off_grad_ckpt)
