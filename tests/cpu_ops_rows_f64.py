"""TEST INFRASTRUCTURE ONLY -- plain f64 references of the row kernels of the denoise step (csrc/elementwise.hip), one
function per kernel.  torch f64 throughout, no cleverness; nothing here imports tests/cpu_ops.py, the oracle or the kernels.

Where a kernel reproduces the reference model's rounding points (QK-RMSNorm: (x * rrms) -> bf16, * scale -> bf16, rotation and
q_mult, ONE rounding) the reference rounds at the same points and keeps everything between two of them in f64.
tests/test_row_kernel_refs.py pins every function here to the project's f32 oracle (oracle/mmdit_oracle.py) on the inputs of
tests/test_gpu_row_kernels.py.
"""
from __future__ import annotations

import math

import torch

F64 = torch.float64
F8 = torch.float8_e4m3fn


def bf16(x: torch.Tensor) -> torch.Tensor:
    """round to the nearest bf16 (ties to even), returned as f64.  (Through f32: a double rounding can only differ from the
    direct one for an f64 value within 2^-29 relative of a bf16 tie -- every comparison here allows one bf16 step anyway.)"""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


# --------------------------------------------------------------------------------------------- LayerNorm + modulate
def ln_modulate_f64(x: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """x [B, L, D], shift / scale [B, D] -> (1 + scale) * LayerNorm(x) + shift, f64, NOT rounded (biased variance, no affine)."""
    x, shift, scale = x.to(F64), shift.to(F64), scale.to(F64)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (1.0 + scale[:, None]) * ((x - mean) / torch.sqrt(var + eps)) + shift[:, None]


def quantize_rows_e4m3(xb: torch.Tensor):
    """xb [M, D] of bf16-representable values -> (e4m3 bytes uint8 [M, D], f32 scales [M]): the quantiser arithmetic of
    tests/test_gpu_fp8.py::_quant_ref (f32: absmax, 448 / absmax, multiply, clamp, one e4m3 rounding)."""
    xf = xb.to(torch.float32)
    amax = xf.abs().amax(-1)
    inv = torch.where(amax > 0, torch.tensor(448.0) / amax, torch.zeros_like(amax))
    q = (xf * inv[:, None]).clamp(-448.0, 448.0).to(F8).view(torch.uint8)
    return q, torch.where(amax > 0, amax / torch.tensor(448.0), torch.ones_like(amax))


def bf16_tie_mask(y: torch.Tensor, window: torch.Tensor) -> torch.Tensor:
    """True where the f64 value y lies within `window` of a bf16 rounding boundary (the midpoint of two neighbouring bf16
    values): arithmetic that is off by less than `window` may round such an element to the other neighbour."""
    ya, ra = y.abs(), bf16(y).abs()
    # the bf16 neighbour of ra on y's side: one step of 2^(e - 7) away, half that towards zero when ra is a power of two
    pow2 = torch.exp2(torch.floor(torch.log2(ra.clamp_min(2.0 ** -126))))
    step = pow2 * 2.0 ** -7
    step = torch.where((ya < ra) & (ra == pow2), 0.5 * step, step)
    mid = ra + torch.sign(ya - ra) * 0.5 * step
    return ((ya - mid).abs() <= window) & (ya != ra)


def ln_modulate_fp8_f64(x, shift, scale, eps: float = 1e-6):
    """osk_ln_modulate_fp8: f64 LayerNorm + modulate, ONE bf16 rounding, then the e4m3 row quantiser.
    Returns (bytes uint8 [M, D], scales f32 [M], tie mask [M, D], rows-with-a-tied-absmax mask [M]).

    tie: the unrounded value is within 16 f32 steps (of the larger of its two terms, the modulated norm and the shift) of a
    bf16 rounding boundary.  The kernel forms mean, rstd, the product and the sum in f32: a handful of roundings of relative
    2^-24 each plus the 1-ulp rsqrt, well inside 16 steps; a value further than that from a boundary rounds to the same bf16
    in f32 and in f64.  A uniformly placed value is a tie with probability 2 * 16 * 2^-24 / 2^-8 ~ 0.05 %."""
    y = ln_modulate_f64(x, shift, scale, eps)
    B, L, D = y.shape
    a = (y - shift.to(F64)[:, None]).abs()
    mag = torch.maximum(a, shift.to(F64)[:, None].abs().expand_as(a))
    window = 16.0 * torch.exp2(torch.floor(torch.log2(mag.clamp_min(2.0 ** -100))) - 23)
    tie = bf16_tie_mask(y, window).reshape(B * L, D)
    yb = bf16(y).reshape(B * L, D)
    q, s = quantize_rows_e4m3(yb)
    # a row's scale may differ when a tie element could be (or stop being) the row's absmax: its other bf16 neighbour is at
    # most one step (2^-7 relative) away
    amax = yb.abs().amax(-1, keepdim=True)
    amax_tie = (tie & (yb.abs() * (1 + 2.0 ** -7) >= amax)).any(-1)
    return q, s, tie, amax_tie


def e4m3_ordinal(b: torch.Tensor) -> torch.Tensor:
    """e4m3 byte -> signed position on the number line (-0 == +0), so that neighbouring codes differ by 1"""
    b = b.to(torch.int32)
    return torch.where(b >= 128, -(b - 128), b)


# --------------------------------------------------------------------------------------------- QK-RMSNorm + RoPE
def qknorm_rope_f64(x, s0, s1, l_split: int, cos, sin, H: int, hd: int, rope_mode: int, eps: float = 1e-6, mult: float = 1.0,
                    with_ties: bool = False):
    """x bf16 [B, L, H * hd]; s0 / s1 bf16 [hd]: the scale vector of positions < l_split / the rest; cos, sin f32 [B or 1, L, hd/2].
    RMSNorm with the reference's two roundings, rotation (mode 0: pairs (2j, 2j+1); mode 1: pairs (j, j + hd/2)) and `mult`
    in f64, one rounding.  Returns f64 [B, L, H * hd] of bf16-representable values.

    with_ties: also returns (tied, extra), both [B, L, H * hd].  tied: the output element's rotation pair holds an element whose
    FIRST rounding, (x * rrms) -> bf16, is a tie: x * rrms lies within 2^-18 relative (64 f32 steps) of a bf16 rounding boundary.
    f32 arithmetic reaches x * rrms through a sum of hd <= 72 squares ((hd - 1) 2^-24 relative at worst, halved by the square
    root), a division, a 1-ulp rsqrt and a product: below 40 * 2^-24 together, so an element that is not tied rounds to the same
    bf16 in f32 and in f64.  (The second rounding needs no such care: the product of two bf16 values is exact in f32.)
    extra: what a tied element rounded the other way moves the output by at most -- one bf16 step of the normalised value times
    the scale (and one more step from re-rounding the product), through |cos| + |sin| <= 2 of the pair, times mult."""
    B, L, _ = x.shape
    xf = x.to(F64).reshape(B, L, H, hd)
    rrms = 1.0 / torch.sqrt((xf * xf).mean(-1, keepdim=True) + eps)
    u = xf * rrms
    t = bf16(u)
    first = (torch.arange(L) < l_split)[None, :, None, None]
    w = torch.where(first, s0.to(F64)[None, None, None, :], s1.to(F64)[None, None, None, :])
    y = bf16(t * w)
    c = cos.to(F64).reshape(-1, L, 1, hd // 2)
    s = sin.to(F64).reshape(-1, L, 1, hd // 2)

    def rotate(a, b):
        if rope_mode == 0:
            return torch.stack((c * a - s * b, s * a + c * b), -1).reshape(B, L, H, hd)
        return torch.cat((a * c - b * s, b * c + a * s), -1)

    def halves(v):
        return (v[..., 0::2], v[..., 1::2]) if rope_mode == 0 else (v[..., : hd // 2], v[..., hd // 2:])

    out = bf16(rotate(*halves(y)) * float(mult)).reshape(B, L, H * hd)
    if not with_ties:
        return out
    tie = bf16_tie_mask(u, u.abs() * 2.0 ** -18)
    # a flipped t moves y by one step of t times the scale, plus at most one step of y from the re-rounding: <= 3 * 2^-8 |y| + ...
    moved = torch.where(tie, 2.0 ** -7 * (t.abs() * w.abs()) + 2.0 ** -7 * y.abs(), torch.zeros_like(y))
    ma, mb = halves(moved)
    pair_moved = ma + mb                           # both outputs of a pair see both of its elements through |cos|, |sin| <= 1
    extra = (torch.stack((pair_moved, pair_moved), -1).reshape(B, L, H, hd) if rope_mode == 0 else torch.cat((pair_moved, pair_moved), -1))
    extra = (extra * abs(float(mult))).reshape(B, L, H * hd)
    return out, extra > 0, extra


# --------------------------------------------------------------------------------------------- V transpose
def vt_key_order(hd: int, Lp: int) -> torch.Tensor:
    """key held at position p of a V^T row, built from the MFMA operand layout csrc/elementwise.hip documents:
    head_dim 72 / 64 (P.V on the 16x16x32 MFMA): the 16-byte chunk c of a 64-key tile belongs to the 32-key half c / 4 and to
    lane row c % 4, and the four lane rows hold the keys {0-3, 8-11}, {16-19, 24-27}, {4-7, 12-15}, {20-23, 28-31};
    head_dim 128 (32x32x16): inside every 16 keys, positions 0-3 -> keys 0-3, 4-7 -> keys 8-11, 8-11 -> keys 4-7, 12-15 -> 12-15."""
    order = []
    if hd in (64, 72):
        lane_rows = [list(range(0, 4)) + list(range(8, 12)), list(range(16, 20)) + list(range(24, 28)),
                     list(range(4, 8)) + list(range(12, 16)), list(range(20, 24)) + list(range(28, 32))]
        for tile in range(Lp // 64):
            for c in range(8):
                order += [64 * tile + 32 * (c // 4) + k for k in lane_rows[c % 4]]
    else:
        in16 = list(range(0, 4)) + list(range(8, 12)) + list(range(4, 8)) + list(range(12, 16))
        for grp in range(Lp // 16):
            order += [16 * grp + k for k in in16]
    return torch.tensor(order, dtype=torch.long)


def v_transpose_ref(v: torch.Tensor, H: int, hd: int) -> torch.Tensor:
    """v [B, L, H * hd] -> [B, H, hd, Lp] in the kernel's key order, keys L .. Lp - 1 zero (same dtype: a pure move)."""
    B, L, _ = v.shape
    Lp = (L + 63) // 64 * 64
    vp = torch.zeros(B, Lp, H, hd, dtype=v.dtype)
    vp[:, :L] = v.reshape(B, L, H, hd)
    return vp[:, vt_key_order(hd, Lp)].permute(0, 2, 3, 1).contiguous()


# --------------------------------------------------------------------------------------------- GEMV task list
def gemv_f64(x: torch.Tensor, layers, act_in: int) -> list:
    """x f32 [Bv, K]; layers: (w bf16 [n, K], bias bf16 [n] | None) -> list of f64 [Bv, n]: (silu(x) if act_in else x) @ w^T + bias"""
    xd = x.to(F64)
    if act_in:
        xd = xd / (1.0 + torch.exp(-xd))
    out = []
    for w, b in layers:
        r = xd @ w.to(F64).T
        out.append(r if b is None else r + b.to(F64))
    return out


# --------------------------------------------------------------------------------------------- timestep embedding, RoPE tables
def timestep_embedding_f64(t: torch.Tensor, dim: int, max_period: float = 10000.0, time_factor: float = 1000.0) -> torch.Tensor:
    """t f32 [B] -> f64 [B, dim]: [cos | sin] of time_factor * t * max_period^(-j / half), an odd dim's last column 0"""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=F64) / half)
    args = float(time_factor) * t.to(F64)[:, None] * freqs[None]
    out = torch.zeros(t.shape[0], dim, dtype=F64)
    out[:, :half] = torch.cos(args)
    out[:, half: 2 * half] = torch.sin(args)
    return out


def rope_angles_f64(ids: torch.Tensor, axes_dim, theta: float) -> torch.Tensor:
    """ids f32 [n, n_axes] -> f64 [n, sum(axes) / 2]: pos * theta^(-2 j / d_axis), the axes side by side"""
    cols = []
    for a, d in enumerate(axes_dim):
        j = torch.arange(0, d, 2, dtype=F64)
        cols.append(ids[:, a].to(F64)[:, None] * torch.pow(torch.tensor(float(theta), dtype=F64), -j / d)[None])
    return torch.cat(cols, -1)


# --------------------------------------------------------------------------------------------- CFG + Euler, row copy
def cfg_euler_f64(pred: torch.Tensor, x: torch.Tensor, g_txt: float, g_img, dt: float) -> torch.Tensor:
    """pred bf16 [3, n] (cond, uncond, uncond_2), x bf16 [n], g_img a float or f32 [n] -> bf16-rounded f64 [n]:
    x + dt * (u2 + g_img (u - u2) + g_txt (c - u))"""
    c, u, u2 = pred.to(F64)
    gi = g_img.to(F64) if torch.is_tensor(g_img) else float(g_img)
    # g_txt, g_img and dt reach the kernel as f32
    gt, dtf = float(torch.tensor(g_txt, dtype=torch.float32)), float(torch.tensor(dt, dtype=torch.float32))
    if not torch.is_tensor(g_img):
        gi = float(torch.tensor(g_img, dtype=torch.float32))
    return bf16(x.to(F64) + dtf * (u2 + gi * (u - u2) + gt * (c - u)))


def copy_rows_ref(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst[j, b, l, :C] = src[j, b, l, :] (src's batch of 1 broadcast) on a copy of dst; the rest of dst unchanged"""
    out = dst.clone()
    out[..., : src.shape[-1]] = src.expand(*dst.shape[:-1], src.shape[-1])
    return out
