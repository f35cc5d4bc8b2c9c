"""Plain-PyTorch restatement of the Video DC-AE DECODER (reference: opensora/models/dc_ae/models/{dc_ae.py, nn/ops.py, nn/norm.py}),
written in our own words as functions over a state dict, so that the GPU tests have a truth where the reference tree does not
exist.  tests/test_dc_ae_host.py pins it against the live reference (when present) and against tests/golden/dc_ae_small.npz, which
tools/make_golden_dc_ae.py records from the reference's own code.

Run in fp32 it is the truth; run in bf16 (parameters and latent cast to bf16) it is the reference-precision comparator of
tests.util.assert_parity: every op keeps the dtype behaviour of the reference (RMSNorm statistics in f32 then a cast back, the
linear attention's matmuls in the tensor's dtype with the division in f32).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

# the golden geometry (ISSUE: widths (32,32,64,64,64,64), depth 1, 32 latent channels) and the shipped one
SMALL = dict(in_channels=3, latent_channels=32, width_list=(32, 32, 64, 64, 64, 64), depth_list=(1, 1, 1, 1, 1, 1),
             block_type=("ResBlock", "ResBlock", "ResBlock", "EViTS5_GLU", "EViTS5_GLU", "EViTS5_GLU"),
             temporal_upsample=(False, False, False, True, True, False))
SHIPPED = dict(in_channels=3, latent_channels=128, width_list=(128, 256, 512, 512, 1024, 1024), depth_list=(3, 3, 3, 3, 3, 3),
               block_type=("ResBlock", "ResBlock", "ResBlock", "EViTS5_GLU", "EViTS5_GLU", "EViTS5_GLU"),
               temporal_upsample=(False, False, False, True, True, False))
DIM = 32          # LiteMLA head dim
EPS_ATT = 1e-15
EPS_NORM = 1e-5


def param_shapes(cfg: dict) -> dict:
    """{state-dict key: shape} of `decoder.*`, in module order"""
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

    conv("decoder.project_in.main", W[-1], cfg["latent_channels"], 3, True)
    for sid in range(n):
        i = 0
        base = f"decoder.stages.{sid}.op_list."
        if sid < n - 1 and D[sid] > 0:
            conv(base + "0.main.conv", W[sid], W[sid + 1], 3, True)
            i = 1
        for _ in range(D[sid]):
            b, c = base + str(i), W[sid]
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
            i += 1
    norm("decoder.project_out.op_list.0", W[0])
    conv("decoder.project_out.op_list.2", cfg["in_channels"], W[0], 3, True)
    return s


def make_state_dict(shapes: dict, seed: int = 0) -> dict:
    """seeded f32 parameters, bf16-representable: conv weights N(0, 1/fan_in), norm scales 1 + 0.1 N, every bias 0.1 N (the
    reference's own trunc_normal init gives outputs near 5e-3; these give O(0.1 .. 0.4))"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k in sorted(shapes):
        shp = tuple(shapes[k])
        x = torch.randn(shp, generator=g)
        if len(shp) == 5:
            x = x / math.sqrt(shp[1] * shp[2] * shp[3] * shp[4])
        elif k.endswith(".weight"):
            x = 1.0 + 0.1 * x
        else:
            x = 0.1 * x
        sd[k] = x.bfloat16().float()
    return {k: sd[k] for k in shapes}


# ---------------------------------------------------------------------------------------------------------------------------
def conv_same(x, w, b=None, groups: int = 1):
    """zero padding of k // 2 on all six faces, then an unpadded conv"""
    p = w.shape[2] // 2
    return F.conv3d(F.pad(x, (p,) * 6) if p else x, w, b, groups=groups)


def conv_same_taps(x, w, b=None, groups: int = 1):
    """conv_same written out as a sum over the k^3 taps, channels last: one matmul per tap (dense), one product per tap
    (depthwise), one batched matmul (grouped 1x1x1).  The same arithmetic in plain torch, with F.conv3d's number format: the sum
    runs in fp32 on the operands as stored and is rounded ONCE to x's dtype (so in bf16 it is neither tighter nor looser a
    comparator than F.conv3d).  For the GPU, where F.conv3d compiles its kernels per shape on first use (minutes for the
    shipped-width tile; seconds through this).  tests/test_dc_ae_host.py pins it to conv_same and to the reference's golden."""
    k = w.shape[2]
    p = k // 2
    B, C, T, H, W = x.shape
    xs = (F.pad(x, (p,) * 6) if p else x).permute(0, 2, 3, 4, 1).float()
    wf = w.float()
    if groups not in (1, C):
        assert k == 1 and w.shape[0] == C
        per = C // groups
        y = torch.einsum("nthwgi,goi->nthwgo", xs.reshape(B, T, H, W, groups, per), wf.reshape(groups, per, per)).reshape(B, T, H, W, C)
    else:
        y = None
        for dt in range(k):
            for dh in range(k):
                for dw in range(k):
                    win = xs[:, dt:dt + T, dh:dh + H, dw:dw + W, :]
                    t = win @ wf[:, :, dt, dh, dw].T if groups == 1 else win * wf[:, 0, dt, dh, dw]
                    y = t if y is None else y.add_(t)
    if b is not None:
        y = y + b.float()
    return y.to(x.dtype).permute(0, 4, 1, 2, 3)


def rms_norm(x, w, b):
    y = (x / torch.sqrt(x.float().square().mean(dim=1, keepdim=True) + EPS_NORM)).to(x.dtype)
    return y * w.view(1, -1, 1, 1, 1) + b.view(1, -1, 1, 1, 1)


def nearest_up(x, temporal: bool):
    if temporal:
        x = x.repeat_interleave(2, dim=2)
    return x.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)


def dup_shortcut(x, cout: int, factor: int, temporal: bool):
    """every input channel repeated `rep` times, then the r^3 (or r^2) consecutive channels of an output channel spread over
    the r x r x r (1 x r x r) block of output voxels"""
    B, C, T, H, W = x.shape
    vol = temporal and T != 1
    rep = cout * factor ** (3 if vol else 2) // C
    x = x.repeat_interleave(rep, dim=1)
    r = factor
    if r == 1:
        return x
    if vol:
        return x.reshape(B, cout, r, r, r, T, H, W).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(B, cout, T * r, H * r, W * r)
    return x.reshape(B, cout, r, r, T, H, W).permute(0, 1, 4, 5, 2, 6, 3).reshape(B, cout, T, H * r, W * r)


def relu_linear_att(qkv):
    B, _, T, H, W = qkv.shape
    if qkv.dtype == torch.float16:
        qkv = qkv.float()
    g = qkv.reshape(B, -1, 3 * DIM, T * H * W)
    q, k, v = F.relu(g[:, :, :DIM]), F.relu(g[:, :, DIM:2 * DIM]), g[:, :, 2 * DIM:]
    v1 = F.pad(v, (0, 0, 0, 1), value=1.0)
    out = (v1 @ k.transpose(-1, -2)) @ q
    if out.dtype == torch.bfloat16:
        out = out.float()
    out = out[:, :, :-1] / (out[:, :, -1:] + EPS_ATT)
    return out.reshape(B, -1, T, H, W)


def decode(sd: dict, cfg: dict, z, taps: bool = False):
    """Decoder.forward on z [B, latent, T, H, W] in z's dtype (sd must hold the same dtype).  taps: every conv through
    conv_same_taps instead of F.conv3d"""
    W, D = cfg["width_list"], cfg["depth_list"]
    n = len(W)

    same = conv_same_taps if taps else conv_same

    def P(key):
        return sd.get(key)

    def conv(key, x, groups=1):
        return same(x, sd[key + ".conv.weight"], P(key + ".conv.bias"), groups)

    x = conv("decoder.project_in.main", z) + dup_shortcut(z, W[-1], 1, False)
    for sid in reversed(range(n)):
        i = 0
        base = f"decoder.stages.{sid}.op_list."
        if sid < n - 1 and D[sid] > 0:
            tu = bool(cfg["temporal_upsample"][sid])
            x = conv(base + "0.main.conv", nearest_up(x, tu and x.shape[2] != 1)) + dup_shortcut(x, W[sid], 2, tu)
            i = 1
        for _ in range(D[sid]):
            b = base + str(i)
            if cfg["block_type"][sid] == "ResBlock":
                h = F.silu(conv(b + ".main.conv1", x))
                h = conv(b + ".main.conv2", h)
                x = x + rms_norm(h, sd[b + ".main.conv2.norm.weight"], sd[b + ".main.conv2.norm.bias"])
            else:
                m = b + ".context_module.main"
                qkv = conv(m + ".qkv", x)
                c3 = qkv.shape[1]
                agg = same(qkv, sd[m + ".aggreg.0.0.weight"], None, groups=c3)
                agg = same(agg, sd[m + ".aggreg.0.1.weight"], None, groups=c3 // DIM)
                both = torch.cat([qkv, agg], dim=1)
                att = relu_linear_att(both).to(both.dtype)
                h = conv(m + ".proj", att)
                x = x + rms_norm(h, sd[m + ".proj.norm.weight"], sd[m + ".proj.norm.bias"])
                m = b + ".local_module.main"
                h = F.silu(conv(m + ".inverted_conv", x))
                h = conv(m + ".depth_conv", h, groups=h.shape[1])
                val, gate = torch.chunk(h, 2, dim=1)
                h = conv(m + ".point_conv", val * F.silu(gate))
                x = x + rms_norm(h, sd[m + ".point_conv.norm.weight"], sd[m + ".point_conv.norm.bias"])
            i += 1
    x = F.relu(rms_norm(x, sd["decoder.project_out.op_list.0.weight"], sd["decoder.project_out.op_list.0.bias"]))
    return conv("decoder.project_out.op_list.2", x)


# ---------------------------------------------------------------------------------------------------------------------------
# the tiled decode (dc_ae.py:589-611, 674-759), restated: overlapping latent tiles, linear cross-fades, crop, concatenate
def crossfade(a, b, extent: int, dim: int):
    """the first `extent` slices of b (along dim) become a mix with the LAST `extent` slices of a; in place in b"""
    extent = min(a.shape[dim], b.shape[dim], extent)
    for e in range(extent):
        ia = [slice(None)] * b.ndim
        ib = [slice(None)] * b.ndim
        ia[dim] = a.shape[dim] - extent + e
        ib[dim] = e
        b[tuple(ib)] = a[tuple(ia)] * (1 - e / extent) + b[tuple(ib)] * (e / extent)
    return b


def tiled_decode(decode_fn, z, *, spatial: bool, temporal: bool, spatial_tile_size: int = 256, temporal_tile_size: int = 32,
                 overlap: float = 0.25, spatial_tile_latent_size: int = 8, temporal_tile_latent_size: int = 8):
    """decode_fn: latent tile -> pixels.  The latent tile sizes are arguments of their own: the reference derives them from its
    CONFIG at construction, not from the (later overridable) pixel tile sizes."""

    def spatial_tiles(zz):
        step = int(spatial_tile_latent_size * (1 - overlap))
        ext = int(spatial_tile_size * overlap)
        keep = spatial_tile_size - ext
        grid = [[decode_fn(zz[..., i:i + spatial_tile_latent_size, j:j + spatial_tile_latent_size])
                 for j in range(0, zz.shape[-1], step)] for i in range(0, zz.shape[-2], step)]
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

    def too_wide(zz):
        return spatial and (zz.shape[-1] > spatial_tile_latent_size or zz.shape[-2] > spatial_tile_latent_size)

    if temporal and z.shape[2] > temporal_tile_latent_size:
        step = int(temporal_tile_latent_size * (1 - overlap))
        ext = int(temporal_tile_size * overlap)
        keep = temporal_tile_size - ext
        parts = []
        for i in range(0, z.shape[2], step):
            zz = z[:, :, i:i + temporal_tile_latent_size]
            parts.append(spatial_tiles(zz) if too_wide(zz) else decode_fn(zz))
        out = []
        for i, t in enumerate(parts):
            if i > 0:
                t = crossfade(parts[i - 1], t, ext, 2)
            out.append(t[:, :, :keep])
        return torch.cat(out, dim=2)
    if too_wide(z):
        return spatial_tiles(z)
    return decode_fn(z)
