"""Plain-PyTorch restatement of the Video DC-AE ENCODER (reference: opensora/models/dc_ae/models/{dc_ae.py:376-440, nn/ops.py,
nn/vo_ops.py}), as functions over a state dict, in the manner of tests/dc_ae_restatement.py, whose helpers (seeded parameters,
zero-padded convs, RMSNorm, linear attention, the cross-fade) it imports.  tests/test_dc_ae_encoder_host.py pins it against the
live reference (when present) and against tests/golden/dc_ae_enc_small.npz, which tools/make_golden_dc_ae_enc.py records from
the reference's own code.

Run in fp32 it is the truth; run in bf16 it is the reference-precision comparator of tests.util.assert_parity.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.dc_ae_restatement import DIM, conv_same, crossfade, make_state_dict, relu_linear_att, rms_norm  # noqa: F401

BLOCKS = ("ResBlock", "ResBlock", "ResBlock", "EViTS5_GLU", "EViTS5_GLU", "EViTS5_GLU")
# the golden geometry (the decoder's small widths, depth 1 everywhere) and the shipped one
SMALL = dict(in_channels=3, latent_channels=32, width_list=(32, 32, 64, 64, 64, 64), depth_list=(1, 1, 1, 1, 1, 1),
             block_type=BLOCKS, temporal_downsample=(False, False, False, True, True, False))
SHIPPED = dict(in_channels=3, latent_channels=128, width_list=(128, 256, 512, 512, 1024, 1024), depth_list=(2, 2, 2, 3, 3, 3),
               block_type=BLOCKS, temporal_downsample=(False, False, False, True, True, False))


def enc_param_shapes(cfg: dict) -> dict:
    """{state-dict key: shape} of `encoder.*`, in module order"""
    W, D = cfg["width_list"], cfg["depth_list"]
    n = len(W)
    s: dict = {}

    def conv(key, co, ci, k, bias):
        s[key + ".conv.weight"] = (co, ci, k, k, k)
        if bias:
            s[key + ".conv.bias"] = (co,)

    def norm(key, c):
        s[key + ".weight"] = (c,)
        s[key + ".bias"] = (c,)

    conv("encoder.project_in", W[0], cfg["in_channels"], 3, True)
    for sid in range(n):
        base = f"encoder.stages.{sid}.op_list."
        c = W[sid]
        for i in range(D[sid]):
            b = base + str(i)
            if cfg["block_type"][sid] == "ResBlock":
                conv(b + ".main.conv1", c, c, 3, True)
                conv(b + ".main.conv2", c, c, 3, False)
                norm(b + ".main.conv2.norm", c)
            else:
                m = b + ".context_module.main"
                conv(m + ".qkv", 3 * c, c, 1, False)
                s[m + ".aggreg.0.0.weight"] = (3 * c, 1, 5, 5, 5)
                s[m + ".aggreg.0.1.weight"] = (3 * c, DIM, 1, 1, 1)
                conv(m + ".proj", c, 2 * c, 1, False)
                norm(m + ".proj.norm", c)
                m = b + ".local_module.main"
                conv(m + ".inverted_conv", 8 * c, c, 1, True)
                s[m + ".depth_conv.conv.weight"] = (8 * c, 1, 3, 3, 3)
                s[m + ".depth_conv.conv.bias"] = (8 * c,)
                conv(m + ".point_conv", c, 4 * c, 1, False)
                norm(m + ".point_conv.norm", c)
        if sid < n - 1 and D[sid] > 0:
            conv(base + f"{D[sid]}.main", W[sid + 1], c, 3, True)
    conv("encoder.project_out.main.op_list.0", cfg["latent_channels"], W[-1], 3, True)
    return s


# ---------------------------------------------------------------------------------------------------------------------------
def conv_strided(x, w, b, stride):
    """zero padding of 1 on all six faces, then an unpadded strided conv"""
    return F.conv3d(F.pad(x, (1,) * 6), w, b, stride=stride)


def avg_shortcut(x, cout: int, factor: int, temporal: bool):
    """the r x r x r (T > 1 and temporal) or 1 x r x r block of voxels of every channel moved into r^3 (r^2) consecutive
    channels, then the mean over groups of consecutive channels"""
    B, C, T, H, W = x.shape
    r = factor
    if temporal and T != 1:
        x = x.reshape(B, C, T // r, r, H // r, r, W // r, r).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(B, C * r ** 3, T // r, H // r, W // r)
    elif r != 1:
        x = x.reshape(B, C, T, H // r, r, W // r, r).permute(0, 1, 4, 6, 2, 3, 5).reshape(B, C * r * r, T, H // r, W // r)
    gs = x.shape[1] // cout
    assert gs * cout == x.shape[1]
    return x.reshape(B, cout, gs, *x.shape[2:]).mean(dim=2)


def res_block(sd, b, x):
    h = F.silu(conv_same(x, sd[b + ".main.conv1.conv.weight"], sd[b + ".main.conv1.conv.bias"]))
    h = conv_same(h, sd[b + ".main.conv2.conv.weight"])
    return x + rms_norm(h, sd[b + ".main.conv2.norm.weight"], sd[b + ".main.conv2.norm.bias"])


def evit_block(sd, b, x):
    m = b + ".context_module.main"
    qkv = conv_same(x, sd[m + ".qkv.conv.weight"])
    c3 = qkv.shape[1]
    agg = conv_same(qkv, sd[m + ".aggreg.0.0.weight"], None, groups=c3)
    agg = conv_same(agg, sd[m + ".aggreg.0.1.weight"], None, groups=c3 // DIM)
    both = torch.cat([qkv, agg], dim=1)
    h = conv_same(relu_linear_att(both).to(both.dtype), sd[m + ".proj.conv.weight"])
    x = x + rms_norm(h, sd[m + ".proj.norm.weight"], sd[m + ".proj.norm.bias"])
    m = b + ".local_module.main"
    h = F.silu(conv_same(x, sd[m + ".inverted_conv.conv.weight"], sd[m + ".inverted_conv.conv.bias"]))
    h = conv_same(h, sd[m + ".depth_conv.conv.weight"], sd[m + ".depth_conv.conv.bias"], groups=h.shape[1])
    val, gate = torch.chunk(h, 2, dim=1)
    h = conv_same(val * F.silu(gate), sd[m + ".point_conv.conv.weight"])
    return x + rms_norm(h, sd[m + ".point_conv.norm.weight"], sd[m + ".point_conv.norm.bias"])


def encode(sd: dict, cfg: dict, x):
    """Encoder.forward on x [B, 3, T, H, W] in x's dtype (sd must hold the same dtype)"""
    W, D = cfg["width_list"], cfg["depth_list"]
    n = len(W)
    x = conv_same(x, sd["encoder.project_in.conv.weight"], sd["encoder.project_in.conv.bias"])
    for sid in range(n):
        base = f"encoder.stages.{sid}.op_list."
        for i in range(D[sid]):
            x = (res_block if cfg["block_type"][sid] == "ResBlock" else evit_block)(sd, base + str(i), x)
        if sid < n - 1 and D[sid] > 0:
            td = bool(cfg["temporal_downsample"][sid])
            k = base + f"{D[sid]}.main.conv."
            x = conv_strided(x, sd[k + "weight"], sd[k + "bias"], (2 if td else 1, 2, 2)) + avg_shortcut(x, W[sid + 1], 2, td)
    k = "encoder.project_out.main.op_list.0.conv."
    return conv_same(x, sd[k + "weight"], sd[k + "bias"]) + avg_shortcut(x, cfg["latent_channels"], 1, False)


# ---------------------------------------------------------------------------------------------------------------------------
# the tiled encode (dc_ae.py:613-672), restated: overlapping PIXEL tiles, cross-fades and crops in LATENT units
def tiled_encode(encode_fn, x, *, spatial: bool, temporal: bool, spatial_tile_size: int = 256, temporal_tile_size: int = 32,
                 overlap: float = 0.25, spatial_tile_latent_size: int = 8, temporal_tile_latent_size: int = 8):
    """encode_fn: pixel tile -> latent.  The latent tile sizes are arguments of their own: the reference derives them from its
    CONFIG at construction, not from the (later overridable) pixel tile sizes."""

    def spatial_tiles(xx):
        step = int(spatial_tile_size * (1 - overlap))
        ext = int(spatial_tile_latent_size * overlap)
        keep = spatial_tile_latent_size - ext
        grid = [[encode_fn(xx[..., i:i + spatial_tile_size, j:j + spatial_tile_size])
                 for j in range(0, xx.shape[-1], step)] for i in range(0, xx.shape[-2], step)]
        out_rows = []
        for i, row in enumerate(grid):
            out = []
            for j, t in enumerate(row):
                if i > 0:
                    t = crossfade(grid[i - 1][j], t, ext, -2)
                if j > 0:
                    t = crossfade(row[j - 1], t, ext, -1)
                out.append(t[..., :keep, :keep])
            out_rows.append(torch.cat(out, dim=-1))
        return torch.cat(out_rows, dim=-2)

    def too_wide(xx):
        return spatial and (xx.shape[-1] > spatial_tile_size or xx.shape[-2] > spatial_tile_size)

    if temporal and x.shape[2] > temporal_tile_size:
        step = int(temporal_tile_size * (1 - overlap))
        ext = int(temporal_tile_latent_size * overlap)
        keep = temporal_tile_latent_size - ext
        parts = []
        for i in range(0, x.shape[2], step):
            xx = x[:, :, i:i + temporal_tile_size]
            parts.append(spatial_tiles(xx) if too_wide(xx) else encode_fn(xx))
        out = []
        for i, t in enumerate(parts):
            if i > 0:
                t = crossfade(parts[i - 1], t, ext, 2)
            out.append(t[:, :, :keep])
        return torch.cat(out, dim=2)
    if too_wide(x):
        return spatial_tiles(x)
    return encode_fn(x)
