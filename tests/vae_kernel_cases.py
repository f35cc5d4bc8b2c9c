"""TEST INFRASTRUCTURE ONLY -- the cases, seeded CPU inputs, f64 references and acceptance checks of the causal 3-D VAE kernel audit
(csrc/conv3d.hip, csrc/conv3d_256.hip; further down: the GroupNorm kernels of csrc/groupnorm.hip and csrc/attention_hd512.hip).

tests/test_gpu_vae_audit.py runs the HIP kernels on these operands and hands their outputs to the check_* functions below;
tests/test_vae_kernel_refs.py hands the SAME functions an f32-accumulated, once-rounded control computed with torch on the SAME
operands -- and mutants of that control -- so the tolerance is shown, without a GPU, to admit f32 arithmetic in another summation
order and to reject small defects.  Inputs come from oracle.synth with fixed seeds, on the CPU.

Reference: the plain statement  upsample -> replicate / causal pad -> conv -> + bias (+ res)  in f64: F.conv3d on the CPU for the
small cases, an unfold-and-matmul in slabs (conv_unfold, on whatever device the operands live on) for the multi-tile cases.  No
kernel of this project is ever the reference.

Tolerance: |out - y| <= 2^-8 |y| + CONV_A max|y|.  2^-8 |y| is exactly one bf16 rounding (unit roundoff 2^-8).  CONV_A is four times the largest
absolute term the f32 control needs on any case (measured by tests/test_vae_kernel_refs.py, recorded in profiles/vae_audit.md):
two independent f32 summation orders differ from each other by up to twice what one differs from f64, doubled again for headroom.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import torch
import torch.nn.functional as F

from tests.row_kernel_cases import rnd

BF = torch.bfloat16
F64 = torch.float64
CONV_REL = 2.0 ** -8
# four times the largest need of the f32 control over every case below (1.155e-7 of max|y|, legacy22_256to256: profiles/vae_audit.md).
# bf16's unit roundoff IS 2^-8, so the relative term is exactly one rounding and the control sits at 0.92 - 0.96 of the bound on every
# case; the absolute term only has to cover what f32 accumulation moves a value across a rounding boundary.  (The cap was 1e-3.)
CONV_A = 4.7e-7
# A conv with the input GroupNorm + SiLU folded in rounds its INPUT twice in the kernel: y = bf16(fma(x, a, d)) -- the f32 fma IS the
# first rounding point, the reference takes it the same way -- then bf16(y / (1 + 2^(-y log2 e))) from f32 arithmetic on v_exp_f32 and
# v_rcp_f32.  That chain is within (4 + |y|) f32 ulps of silu(y): 1 ulp each for exp and rcp, half an ulp for each of the add and the
# two multiplies, and the rounding of t = -y log2 e moves 2^t by |y| 2^-24 relative.  So the kernel may round bf16(silu(y)) the other
# way exactly where silu(y) lies within that margin of a bf16 rounding boundary -- a property of the value of y, decided here in
# f64 (gn_in_slack).  An output's bound grows by the sum over ITS near-boundary inputs of |w| x one bf16 step of that input: a
# per-element term (on average 2e-6 of max|y|), nothing for the elements that see no such input.  The whole absolute term is
# clamped to ABS_CAP max|y|.  The f32 control (gn_in_input_f32) runs the same chain with torch's exp2 and reciprocal.
ABS_CAP = 1e-3
STATS_REL = 2e-5                  # fused statistics: f32 partials per tile, f64 across tiles (tests/test_gpu_vae.py's rule)
CUS_ASSUMED = 256                 # without a device (the host-only report assumes the same)

CLASSES = ("tile128", "tile128_bigc", "fewout", "conv256x4", "conv256x8", "convsw4", "convsw8", "convsw4_up", "convsw8_up",
           "convsw8_gn", "convsw2", "convsw2_gn")
STATS_CLASSES = CLASSES[3:]       # the large-tile kernels: their epilogue can carry gn_sums


class ConvCase(NamedTuple):
    id: str
    cls: str                      # the kernel class the call must reach (osk_causal_conv3d_kernel_class)
    edge: str                     # what the case exists for
    Cin: int
    Cout: int
    k: int = 3
    stride: tuple = (1, 1, 1)
    up: tuple = (False, False)
    B: int = 1
    T: int = 2
    H: int = 16
    W: int = 16
    res: bool = False
    out_off: int = 0              # bf16 elements `out` starts past a 16-byte boundary (4 = 8-byte aligned only)
    res_off: int = 0
    gn_G: int = 0                 # > 0: the case ALSO runs with gn_sums (that many groups) and must come back fused
    gn_in: bool = False
    multi: str = ""               # multi-tile case: extents come from multi_extent(kind, CUs)
    structured: bool = False      # one-hot x, ramp w, bit-exact
    repeat: bool = False          # run three times, bit-equal


def _c(id, cls, edge, Cin, Cout, **kw):
    return ConvCase(id, cls, edge, Cin, Cout, **kw)


def _legacy():
    """tests/test_gpu_vae.py::CONV_CASES as they are, each with the class it reaches (until now a comment there was the only record)"""
    from tests.test_gpu_vae import CONV_CASES
    cls = ["tile128", "tile128", "tile128_bigc", "tile128_bigc", "conv256x4", "tile128_bigc", "tile128_bigc", "tile128_bigc", "tile128",
           "tile128", "tile128_bigc", "tile128_bigc", "tile128_bigc", "conv256x8", "conv256x4", "conv256x4", "conv256x8", "conv256x8",
           "convsw8_up", "fewout", "fewout", "convsw2", "convsw8", "convsw8", "convsw4", "convsw4", "convsw2", "convsw8_up", "convsw4_up",
           "convsw8_up"]
    assert len(cls) == len(CONV_CASES)
    out = []
    for i, (c, k) in enumerate(zip(CONV_CASES, cls)):
        ci, co, ks, stride, up, B, T, H, W, res = c
        cip = 8
        while cip < ci:
            cip *= 2
        out.append(_c(f"legacy{i:02d}_{ci}to{co}", k, "CONV_CASES of tests/test_gpu_vae.py", cip, co, k=ks, stride=stride, up=up, B=B, T=T,
                      H=H, W=W, res=res))
    return out


UP_TT, UP_HW = (True, True), (False, True)
NEW_CASES = [
    # ---- generic (per-element) epilogue of the large-tile kernels: Cout % 16 != 0, or out / res only 8-byte aligned
    _c("gen_x4_co136", "conv256x4", "Cout 136: tail inside a 16-channel block, ragged M (260)", 128, 136, H=10, W=13),
    _c("gen_x8_co264", "conv256x8", "Cout 264: tail inside a 16-channel block of the second 256-tile, residual", 128, 264, H=10, W=13, res=True),
    _c("gen_x4_co200_res", "conv256x4", "Cout 200 with residual, ragged M", 128, 200, H=10, W=13, res=True),
    _c("gen_x4_co200", "conv256x4", "Cout 200 without residual, ragged M", 128, 200, H=10, W=13),
    _c("gen_x8_co328_res", "conv256x8", "Cout 328 (256 + 72) with residual, ragged M", 128, 328, H=10, W=13, res=True),
    _c("gen_x4_out8", "conv256x4", "Cout % 16 == 0, out 8- but not 16-byte aligned", 128, 160, H=10, W=13, res=True, out_off=4),
    _c("gen_x4_res8", "conv256x4", "Cout % 16 == 0, res 8- but not 16-byte aligned", 128, 160, H=10, W=13, res=True, res_off=4),
    _c("gen_x8_out8", "conv256x8", "Cout % 16 == 0, out 8- but not 16-byte aligned", 128, 256, H=10, W=13, out_off=4),
    _c("gen_x8_res8", "conv256x8", "Cout % 16 == 0, res 8- but not 16-byte aligned", 128, 256, H=10, W=13, res=True, res_off=4, repeat=True),
    _c("gen_sw2_out8", "convsw2", "two-frame form through the generic epilogue (out 8-byte aligned), odd T", 128, 128, T=3, out_off=4),
    _c("gen_sw4_co136", "convsw4", "sliding window through the generic epilogue: Cout 136, weight rows clamped inside a piece", 128, 136),
    # ---- sliding-window kernels with an odd number of 32-channel blocks
    _c("sw4_co160", "convsw4", "Cout 160 = five 32-channel blocks: the second 128-tile holds one", 128, 160),
    _c("sw8_co288", "convsw8", "Cout 288 = nine blocks, 16 x 32: the second 256-tile holds one", 128, 288, W=32, res=True),
    _c("sw4up_co160", "convsw4_up", "Cout 160 under the folded upsample", 128, 160, up=UP_TT, H=8, W=8),
    _c("sw8up_co288", "convsw8_up", "Cout 288 under the folded upsample, 16 x 32 output", 128, 288, up=UP_TT, H=8, W=16, res=True),
    # ---- few-output kernel: NC = 1, 2; Ho = 5 -> the last group of 4 rows is partial
    _c("fewout1", "fewout", "conv_fewout_kernel<1>, partial last row group", 128, 1, H=5, W=64),
    _c("fewout2", "fewout", "conv_fewout_kernel<2>, partial last row group, residual", 128, 2, H=5, W=64, res=True),
    # ---- two-frame form across batch items: the last pair of item 0 has one frame, the next tile belongs to item 1
    _c("sw2_B2_T3", "convsw2", "B 2, T 3", 128, 128, B=2, T=3, gn_G=32),
    _c("sw2_B2_T5", "convsw2", "B 2, T 5, residual", 128, 128, B=2, T=5, res=True, repeat=True),
    # ---- upsampling kernels: single frame (image decode), H, W only, batch
    _c("sw8up_T1", "convsw8_up", "T 1 with up_t set: Tu = To = 1", 128, 256, up=UP_TT, T=1, H=8, W=8),
    _c("sw4up_T1", "convsw4_up", "T 1 with up_t set: Tu = To = 1", 128, 128, up=UP_TT, T=1, H=8, W=8),
    _c("sw8up_hw", "convsw8_up", "H, W upsample only", 128, 256, up=UP_HW, H=8, W=8),
    _c("sw4up_B2", "convsw4_up", "B 2 with up_t: frame 0 of EACH item is the un-doubled one", 128, 128, up=UP_TT, B=2, H=8, W=8, gn_G=32),
    _c("sw8up_B2", "convsw8_up", "B 2 with up_t", 128, 256, up=UP_TT, B=2, H=8, W=8, res=True, gn_G=16),
    # ---- fused statistics on B = 2 with per_b % 256 == 0 (classes the multi-tile cases do not reach)
    _c("x8_B2_stats", "conv256x8", "B 2, per_b = 256, 8 channels per group", 128, 256, B=2, H=16, W=8, gn_G=32),
    _c("x4_B2_stats", "conv256x4", "B 2, per_b = 256, 16 channels per group, residual", 128, 160, B=2, H=16, W=8, res=True, gn_G=10),
    _c("sw4_B2_stats", "convsw4", "B 2, Cout 160, 8 channels per group", 128, 160, B=2, T=1, gn_G=20),
    # ---- the input GroupNorm + SiLU folded in
    _c("sw8gn_co288", "convsw8_gn", "Cout 288 (nine blocks), residual", 128, 288, gn_in=True, res=True),
    _c("sw2gn_B2_T3", "convsw2_gn", "B 2, T 3: one table per item, the last pair of item 0 has one frame", 128, 128, B=2, T=3, gn_in=True, gn_G=32),
    # ---- more tiles than CUs with a partial last round, compared in full (extents from the CU count)
    _c("multi_x4", "conv256x4", "ntiles > CUs, partial last round, ragged M", 128, 128, multi="x", gn_G=32, repeat=True),
    _c("multi_x8", "conv256x8", "ntiles > CUs, partial last round, ragged M", 128, 256, multi="x", res=True, gn_G=32, repeat=True),
    _c("multi_sw4", "convsw4", "ntiles > CUs, single frame", 128, 128, multi="sw1", repeat=True),
    _c("multi_sw8", "convsw8", "ntiles > CUs", 128, 256, multi="sw", gn_G=16, repeat=True),
    _c("multi_sw2", "convsw2", "ntiles > CUs, odd T", 128, 128, multi="sw2", res=True, gn_G=32, repeat=True),
    _c("multi_sw8up", "convsw8_up", "ntiles > CUs", 128, 256, multi="swup", up=UP_TT, gn_G=32, repeat=True),
    _c("multi_sw8gn", "convsw8_gn", "ntiles > CUs", 128, 256, multi="sw", gn_in=True, gn_G=16, repeat=True),
    # ---- structured, transpose-detecting, bit-exact: one per class
    _c("exact_tile128", "tile128", "structured", 32, 64, T=3, H=9, W=7, structured=True),
    _c("exact_tile128_bigc", "tile128_bigc", "structured, strided", 64, 64, stride=(1, 2, 2), T=4, H=11, W=13, structured=True),
    _c("exact_fewout", "fewout", "structured", 128, 3, H=5, W=64, structured=True),
    _c("exact_x4", "conv256x4", "structured, generic epilogue", 128, 136, H=10, W=13, structured=True),
    _c("exact_x8", "conv256x8", "structured, strided in time", 128, 256, stride=(2, 1, 1), T=5, H=10, W=13, structured=True),
    _c("exact_sw4", "convsw4", "structured", 128, 160, structured=True),
    _c("exact_sw8", "convsw8", "structured, two body iterations", 256, 288, structured=True),
    _c("exact_sw4_up", "convsw4_up", "structured", 128, 128, up=UP_TT, H=8, W=8, structured=True),
    _c("exact_sw8_up", "convsw8_up", "structured, H, W only", 128, 256, up=UP_HW, H=8, W=16, structured=True),
    _c("exact_sw8_gn", "convsw8_gn", "structured", 128, 256, gn_in=True, structured=True),
    _c("exact_sw2", "convsw2", "structured, odd T", 128, 128, T=3, structured=True),
    _c("exact_sw2_gn", "convsw2_gn", "structured", 128, 128, T=4, gn_in=True, structured=True),
]
CONV_CASES = _legacy() + NEW_CASES
CASE = {c.id: c for c in CONV_CASES}
assert len(CASE) == len(CONV_CASES)


def out_dims(T, H, W, stride, up):
    Tu = 1 + 2 * (T - 1) if up[0] else T
    Hu, Wu = (2 * H, 2 * W) if up[1] else (H, W)
    return (Tu - 1) // stride[0] + 1, (Hu - 1) // stride[1] + 1, (Wu - 1) // stride[2] + 1


def _units(cus: int, per: int) -> int:
    """smallest n with n * per tiles > cus + 2 and n * per no multiple of cus"""
    n = (cus + 3 + per - 1) // per
    while (n * per) % cus == 0:
        n += 1
    return n


def multi_extent(c: ConvCase, cus: int):
    """(B, T, H, W, ntiles) of a multi-tile case on a part with `cus` compute units: more tiles than CUs, the last round partial"""
    ncol = (c.Cout + 255) // 256 if c.Cout >= 256 else (c.Cout + 127) // 128
    if c.multi == "x":          # linear 256-voxel tiles, W = 24 (no whole bricks), T = 2: M = 48 H just past cus + 2 tiles, ragged
        H = ((cus + 2) * 256) // 48 + 1
        B, T, W = 1, 2, 24
        ntiles = (2 * H * W + 255) // 256
    elif c.multi == "sw1":      # one frame, one row of bricks
        B, T, H = 1, 1, 16
        ntiles = _units(cus, 1)
        W = 16 * ntiles
    elif c.multi == "sw":       # two frames per brick
        B, T, H = 1, 2, 16
        n = _units(cus, 2)
        W, ntiles = 16 * n, 2 * n
    elif c.multi == "sw2":      # T = 3: two frame pairs per brick, the second holds one frame
        B, T, H = 1, 3, 16
        n = _units(cus, 2)
        W, ntiles = 16 * n, 2 * n
    elif c.multi == "swup":     # source T = 2 -> 3 output frames per 16 x 16 output brick (8 x 8 source)
        B, T, H = 1, 2, 8
        n = _units(cus, 3)
        W, ntiles = 8 * n, 3 * n
    else:
        raise ValueError(c.multi)
    ntiles *= ncol
    assert ntiles > cus and ntiles % cus != 0, (c.id, ntiles, cus)
    return B, T, H, W, ntiles


def shape_of(c: ConvCase, cus: int = CUS_ASSUMED):
    return multi_extent(c, cus)[:4] if c.multi else (c.B, c.T, c.H, c.W)


# ============================================================================================= operands
def _structured(c: ConvCase, B, T, H, W):
    """x one-hot in channel on a lattice of positions 3 apart (t = 1 mod 3, h = 1 mod 3, w = 1 mod 3, never on a replicated border
    when the extent allows), another channel at every lattice point; w an asymmetric ramp over [Cout][tap][Cin].  Without the
    upsample every output is ONE weight (modulus 251); under the upsample a source point is seen through up to 8 taps, so the
    modulus is 29 and every sum stays an integer below 256: exact in bf16 either way.  A swapped tap order, channel chunk or
    (h, w) reads back as another integer."""
    x = torch.zeros(B, T, H, W, c.Cin)
    ts = [t for t in range(T) if t % 3 == 1] or [0]
    hs = [h for h in range(1, max(H - 1, 2)) if h % 3 == 1]
    ws = [w for w in range(1, max(W - 1, 2)) if w % 3 == 1]
    for b in range(B):
        for t in ts:
            for h in hs:
                for w in ws:
                    x[b, t, h, w, (37 * t + 11 * h + 5 * w + 3 * b) % c.Cin] = 1.0
    K = c.k ** 3 * c.Cin
    mod = 29 if (c.up[0] or c.up[1]) else 251
    wk = (torch.arange(c.Cout * K, dtype=torch.int64) % mod).reshape(c.Cout, K).float()
    return x, wk


@functools.lru_cache(maxsize=4)
def operands(cid: str, cus: int = CUS_ASSUMED):
    """CPU operands of a case: x bf16 [B, T, H, W, Cin], w bf16 [Cout, Kpad] (tap-major, channel-minor), bias f32, res bf16 | None,
    table f32 [B, Cin / 8, 16] | None (the folded GroupNorm's scales and shifts: an INPUT of the conv)"""
    c = CASE[cid]
    B, T, H, W = shape_of(c, cus)
    To, Ho, Wo = out_dims(T, H, W, c.stride, c.up)
    K = c.k ** 3 * c.Cin
    Kp = (K + 63) // 64 * 64
    if c.structured:
        x, wk = _structured(c, B, T, H, W)
        bias = torch.zeros(c.Cout)
    else:
        x = rnd(f"vae.x.{cid}", (B, T, H, W, c.Cin), seed=311).float()
        wk = rnd(f"vae.w.{cid}", (c.Cout, K), std=K ** -0.5, seed=312).float()
        bias = rnd(f"vae.b.{cid}", (c.Cout,), std=0.1, seed=313).float()
    w = torch.zeros(c.Cout, Kp)
    w[:, :K] = wk
    res = rnd(f"vae.r.{cid}", (B, To, Ho, Wo, c.Cout), seed=314) if c.res else None
    table = None
    if c.gn_in:
        table = torch.zeros(B, c.Cin // 8, 16)
        if c.structured:
            table[:, :, :8] = 1.0          # y = x: silu(1) rounds to 187 / 256, every product stays an exact f32
        else:
            a = 1.0 + 0.3 * rnd(f"vae.ga.{cid}", (B, c.Cin), seed=315, dtype=torch.float32)
            d = 0.3 * rnd(f"vae.gd.{cid}", (B, c.Cin), seed=316, dtype=torch.float32)
            table[:, :, :8] = a.reshape(B, -1, 8)
            table[:, :, 8:] = d.reshape(B, -1, 8)
    return dict(case=c, B=B, T=T, H=H, W=W, To=To, Ho=Ho, Wo=Wo, x=x.to(BF), w=w.to(BF), bias=bias, res=res, table=table)


def gn_in_input(x: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """f64: what the conv sees with the GroupNorm + SiLU folded in, rounded at the kernel's two rounding points:
    bf16(silu(bf16(x a + d)))"""
    B, C = x.shape[0], x.shape[-1]
    a = table[:, :, :8].reshape(B, 1, 1, 1, C).to(x.device).double()
    d = table[:, :, 8:].reshape(B, 1, 1, 1, C).to(x.device).double()
    y = (x.double() * a + d).to(BF).double()
    return (y * torch.sigmoid(y)).to(BF).double()


def gn_in_input_f32(x: torch.Tensor, table: torch.Tensor, mutant: str = "") -> torch.Tensor:
    """the control's input: the same two roundings from f32 arithmetic, in the kernel's order of operations --
    y = bf16(fma(x, a, d)); out = bf16(y * (1 / (1 + 2^(-y log2 e)))), every step rounded to f32 (the fma through f64: x a is exact
    there)."""
    B, C = x.shape[0], x.shape[-1]
    if mutant == "gn_table_chunk":         # the scales and shifts of the neighbouring 8-channel chunk
        table = torch.roll(table, 1, 1)
    a = table[:, :, :8].reshape(B, 1, 1, 1, C).double()
    d = table[:, :, 8:].reshape(B, 1, 1, 1, C).double()
    y = (x.double() * a + d).float()
    if mutant != "gn_single_rounding":     # y not rounded to bf16 before the SiLU
        y = y.to(BF).float()
    nl2e = torch.tensor(-1.4426950408889634, dtype=torch.float32)
    return (y * torch.reciprocal(1.0 + torch.exp2(y * nl2e))).to(BF)


def gn_in_slack(o, device="cpu", voxels=None) -> torch.Tensor:
    """f64 [n, Cout]: per output, the sum over its inputs whose silu(y) lies within (4 + |y|) f32 ulps of a bf16 rounding boundary
    of |w| x the bf16 step to the value on the other side (see ABS_CAP above)"""
    c = o["case"]
    x, table = o["x"].to(device), o["table"].to(device)
    B, C = x.shape[0], x.shape[-1]
    a = table[:, :, :8].reshape(B, 1, 1, 1, C).double()
    d = table[:, :, 8:].reshape(B, 1, 1, 1, C).double()
    y = (x.double() * a + d).float().to(BF).double()
    s = y * torch.sigmoid(y)
    r = s.float().to(BF)
    ri = r.view(torch.int16).to(torch.int32)
    rd = r.double()
    margin = (4 + y.abs()) * 2.0 ** -24 * s.abs()
    step = torch.zeros_like(s)
    for nb in (ri + 1, ri - 1):            # the bf16 neighbours of r: the boundary is half way
        other = nb.to(torch.int16).view(BF).double()
        near = (s - (rd + other) / 2).abs() <= margin
        step = torch.where(near, torch.maximum(step, (other - rd).abs()), step)
    return conv_unfold(step, o["w"].to(device).double().abs(), None, None, c, F64, voxels)


# ============================================================================================= the plain statement
def upsample(xs: torch.Tensor, up, mutant: str = "") -> torch.Tensor:
    """nearest 2x on [B, T, H, W, C]: frame 0 stays single under up_t (UpsampleCausal3D)"""
    if up[0]:
        if mutant == "frame0_doubled":
            xs = xs.repeat_interleave(2, 1)[:, : 2 * xs.shape[1] - 1]
        else:
            xs = torch.cat((xs[:, :1], xs[:, 1:].repeat_interleave(2, 1)), 1)
    if up[1]:
        if mutant == "up_index":       # source row (h + 1) >> 1 instead of h >> 1
            H = xs.shape[2]
            idx = ((torch.arange(2 * H, device=xs.device) + 1) >> 1).clamp(max=H - 1)
            xs = xs[:, :, idx].repeat_interleave(2, 3)
        else:
            xs = xs.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return xs


def pad(xs: torch.Tensor, k: int, mutant: str = "") -> torch.Tensor:
    """replicate padding H, W by k // 2 on both sides, T by k - 1 in FRONT (causal), on [B, T, H, W, C]"""
    if k == 1:
        return xs
    v = xs.permute(0, 4, 1, 2, 3)
    tp = (1, 1) if mutant == "symmetric_time" else (2, 0)
    v = F.pad(v, (1, 1, 1, 1) + tp, mode="replicate").permute(0, 2, 3, 4, 1).contiguous()
    if mutant == "zero_face":          # zero instead of replicate at the w = -1 face
        v[:, :, :, 0] = 0
    return v


def conv_unfold(x, w, bias, res, c: ConvCase, dtype=F64, voxels=None, mutant: str = "", slab: int = 8192):
    """the plain statement as unfold-and-matmul in `dtype`, in slabs of output voxels, on x's device -> [n, Cout] for the linear
    output voxel indices `voxels` (default: all, in [B, To, Ho, Wo] order).  dtype f64 = the reference of the multi-tile cases;
    f32 = the control (one summation order of f32, the caller rounds once to bf16).  `mutant` plants one defect (refs test)."""
    dev = x.device
    k, (st, sh, sw) = c.k, c.stride
    B, T, H, W, Cin = x.shape
    To, Ho, Wo = out_dims(T, H, W, c.stride, c.up)
    xs = pad(upsample(x.to(dtype), c.up, mutant), k, mutant)
    K = k ** 3 * Cin
    wk = w[:, :K].to(dtype)
    if mutant == "tap_chunk":          # tap 14's weights dropped for the 8-channel chunk 3 (the 16-byte unit a lane loads)
        wk = wk.clone()
        t0 = (14 if k == 3 else 0) * Cin + 24
        wk[:, t0: t0 + 8] = 0
    r = None if res is None else res.to(dtype)
    if mutant == "res_neighbour" and r is not None:
        r = torch.roll(r, 1, 3)
    M = B * To * Ho * Wo
    vox = torch.arange(M, device=dev) if voxels is None else voxels.to(dev)
    out = torch.empty(vox.numel(), c.Cout, dtype=dtype, device=dev)
    taps = [(dt, dh, dw) for dt in range(k) for dh in range(k) for dw in range(k)]
    for s in range(0, vox.numel(), slab):
        m = vox[s: s + slab]
        wo, q = m % Wo, m // Wo
        ho, q = q % Ho, q // Ho
        to, b = q % To, q // To
        cols = torch.stack([xs[b, to * st + dt, ho * sh + dh, wo * sw + dw] for dt, dh, dw in taps], 1).reshape(m.numel(), K)
        y = cols @ wk.T
        if bias is not None:
            y = y + bias.to(dev).to(dtype)
        if r is not None:
            y = y + r.reshape(M, c.Cout)[m]
        out[s: s + slab] = y
    return out


def conv_ref_small(o) -> torch.Tensor:
    """F.conv3d in f64 on the CPU -> [M, Cout]"""
    c = o["case"]
    x = gn_in_input(o["x"], o["table"]) if c.gn_in else o["x"].double()
    xs = pad(upsample(x, c.up), c.k).permute(0, 4, 1, 2, 3)
    K = c.k ** 3 * c.Cin
    wk = o["w"][:, :K].double().reshape(c.Cout, c.k, c.k, c.k, c.Cin).permute(0, 4, 1, 2, 3)
    y = F.conv3d(xs, wk, o["bias"].double(), stride=c.stride).permute(0, 2, 3, 4, 1)
    if o["res"] is not None:
        y = y + o["res"].double()
    return y.reshape(-1, c.Cout)


def sample_voxels(M: int, n: int = 384) -> torch.Tensor:
    """the CPU's share of a multi-tile case: first and last voxels, both sides of 256-voxel tile edges, a spread in between"""
    g = torch.Generator().manual_seed(M)
    idx = torch.cat((torch.arange(8), torch.arange(M - 8, M), torch.tensor([255, 256, 257, M // 2, M // 2 + 1]),
                     torch.randint(0, M, (n,), generator=g)))
    return idx.clamp(0, M - 1).unique()


def reference(o, device="cpu", voxels=None) -> torch.Tensor:
    """f64 [n, Cout].  Small cases: F.conv3d on the CPU.  Multi-tile cases: conv_unfold on `device` (the operands are moved there)."""
    c = o["case"]
    if not c.multi:
        y = conv_ref_small(o)
        return y if voxels is None else y[voxels]
    x = o["x"].to(device)
    x = gn_in_input(x, o["table"]) if c.gn_in else x
    return conv_unfold(x, o["w"].to(device), o["bias"], None if o["res"] is None else o["res"].to(device), c, F64, voxels)


def control(o, voxels=None, mutant: str = "") -> torch.Tensor:
    """f32-accumulated, once-rounded: what a correct kernel with another summation order looks like (bf16 [n, Cout], CPU)"""
    c = o["case"]
    x = gn_in_input_f32(o["x"], o["table"], mutant) if c.gn_in else o["x"]
    return conv_unfold(x, o["w"], o["bias"], o["res"], c, torch.float32, voxels, mutant).to(BF)


# ============================================================================================= checks
def conv_need(got: torch.Tensor, ref: torch.Tensor) -> float:
    """the absolute term the comparison needs, relative to max|y| (row_kernel_cases.excess / max|y|)"""
    g, r = got.double(), ref.double()
    return float(((g - r).abs() - CONV_REL * r.abs()).max() / r.abs().max())


def check_conv(got: torch.Tensor, ref: torch.Tensor, o, what: str = "", slack=None) -> float:
    """got bf16 [n, Cout] against the f64 reference [n, Cout]: every element, finite, within the bound; structured cases bit for
    bit.  Prints err / tol (worst element) and the absolute term needed before it asserts; returns the ratio."""
    c = o["case"]
    g, r = got.double().cpu(), ref.double().cpu()
    assert g.shape == r.shape, (g.shape, r.shape)
    assert bool(torch.isfinite(g).all()), f"{c.id}: non-finite output"
    if c.structured:
        want = r.to(BF)      # (every f32 partial sum is exact, so the kernel rounds the same exact value once)
        assert c.gn_in or bool((want.double() == r).all()), "the structured expectation must be exact in bf16"
        bad = int((got.cpu().view(torch.int16) != want.view(torch.int16)).sum())
        print(f"{what}{c.id} [{c.cls}] structured: {bad} of {g.numel()} elements differ (bit-exact required)")
        assert bad == 0, f"{c.id}: {bad} elements are not the expected weight"
        return 0.0
    ymax = float(r.abs().max())
    tol_abs = CONV_A * ymax
    if c.gn_in:         # + the per-element slack of the near-boundary inputs (gn_in_slack); required for these cases
        sl = slack.double().cpu()
        print(f"{what}{c.id} GN-in slack: max {float(sl.max()) / ymax:.3e}, mean {float(sl.mean()) / ymax:.3e} of max|y|")
        tol_abs = torch.clamp(tol_abs + sl, max=ABS_CAP * ymax)      # never above the cap, whatever the extent's unluckiest element
    tol = CONV_REL * r.abs() + tol_abs
    ratio = float(((g - r).abs() / tol).max())
    print(f"{what}{c.id} [{c.cls}] err/tol {ratio:.3f}, abs term needed {conv_need(g, r):.3e} of max|y| (allowed {CONV_A:.1e})")
    assert ratio <= 1.0, f"{c.id}: err/tol {ratio:.3f}"
    return ratio


def stats_exact(out: torch.Tensor, B: int, G: int):
    """f64 (sum, sum of squares) per (batch, group) of the bf16 output [B, ..., Cout] and the cancellation-free magnitude of each"""
    C = out.shape[-1]
    xf = out.double().reshape(B, -1, G, C // G)
    exact = torch.stack((xf.sum((1, 3)), (xf * xf).sum((1, 3))), -1)
    scale = torch.stack((xf.abs().sum((1, 3)), (xf * xf).sum((1, 3))), -1)
    return exact, scale


def check_stats(sums: torch.Tensor, out: torch.Tensor, B: int, G: int, cid: str) -> float:
    exact, scale = stats_exact(out, B, G)
    ratio = float(((sums.double().to(exact.device) - exact).abs() / (STATS_REL * scale + 1e-9)).max())
    print(f"{cid} fused statistics (G {G}): err/tol {ratio:.3f}")
    assert ratio <= 1.0, f"{cid}: fused statistics err/tol {ratio:.3f}"
    return ratio


def report_args(o, *, stats: bool = False):
    """keyword arguments of _C.conv_kernel_class for the call the audit makes"""
    c = o["case"]
    return dict(B=o["B"], T=o["T"], H=o["H"], W=o["W"], Cin=c.Cin, Cout=c.Cout, ksize=c.k, stride=c.stride, up=c.up,
                out_align=8 if c.out_off else 16, res_align=0 if not c.res else (8 if c.res_off else 16),
                gn_groups=c.gn_G if stats else 0, gn_in=c.gn_in)


# mutants of the control every check must reject, and the cases they are planted in (cases where the defect is reachable)
MUTANTS = {
    "tap_chunk": ["gen_x4_co136", "sw8_co288", "legacy01_32to64", "fewout2", "sw8gn_co288", "multi_sw8gn"],
    "zero_face": ["gen_x4_co200", "sw4_co160", "sw8up_T1", "sw8gn_co288"],
    "symmetric_time": ["gen_x8_co264", "sw2_B2_T3", "sw4up_B2", "sw2gn_B2_T3"],
    "gn_table_chunk": ["sw8gn_co288", "sw2gn_B2_T3", "multi_sw8gn"],
    "gn_single_rounding": ["sw8gn_co288", "sw2gn_B2_T3"],
    "up_index": ["sw4up_co160", "sw8up_hw", "legacy04_128to128"],
    "frame0_doubled": ["sw8up_B2", "sw4up_B2", "legacy17_256to256"],
    "res_neighbour": ["gen_x4_co200_res", "sw2_B2_T5", "sw8up_co288", "fewout2", "sw8gn_co288"],
}


# ============================================================================================= GroupNorm kernels (csrc/groupnorm.hip)
# class edges: channels per group 1 .. 16 (the shuffle reduction of gn_stats has log2(cpg) steps), and S of 1, 1023, 1025 and 2500:
# one voxel; one short of / one past 1024 rows (C = 32: the rows of one stats pass); and an S that leaves the last block of both
# grids a partial slab at every C (stats blocks hold max(4 rpp, ceil(S / 256)) rows, rpp = 8192 / C)
GN_CG = [(32, 32), (64, 32), (128, 32), (256, 32), (512, 32), (32, 2)]       # cpg 1, 2, 4, 8, 16, 16
GN_S = [1, 1023, 1025, 2500]
GN_B = 2
GN_EPS = 1e-6
GN_CASES = [(C, G, S) for C, G in GN_CG for S in GN_S]
# |mean| * rstd of the large-mean statistics case: twice the largest any GroupNorm input shows in the full-size config-3 encode and
# decode with the synthetic weights (profiles/vae_audit.md)
GN_BIG_RATIO = 1.18    # 2 x 0.586 (encoder, C 256, S 69632; the decoder's largest is 0.506), rounded up
GN_BIG_CASE = (128, 32, 65536)     # 256 stats blocks of 256 rows: four rows per thread, the kernel's floor
# share of gn_apply outputs that may differ at all from the f64 statement: twice the pooled share of the f32 control over GN_CASES,
# with and without SiLU (1031 of 18632704, tests/test_vae_kernel_refs.py)
GN_SHARE_CAP = 2 * 1031 / 18632704
GN_RSTD_REL = 2.0 ** -10


@functools.lru_cache(maxsize=None)
def gn_case(C: int, G: int, S: int, ratio: float = 0.0):
    """x bf16 [B, S, C], gamma / beta f32, the f64 sums, mean, rstd and the f64 apply output rounded at the kernel's two rounding
    points (with and without SiLU).  ratio > 0: the mean is moved to ratio standard deviations."""
    x = rnd(f"gn.x.{C}.{G}.{S}", (GN_B, S, C), std=1.5, seed=321, mean=0.7 if not ratio else 1.5 * ratio)
    gamma = 1.0 + rnd(f"gn.g.{C}", (C,), std=0.2, seed=322, dtype=torch.float32)
    beta = rnd(f"gn.b.{C}", (C,), std=0.2, seed=323, dtype=torch.float32)
    xg = x.double().reshape(GN_B, S, G, C // G)
    sums = torch.stack((xg.sum((1, 3)), (xg * xg).sum((1, 3))), -1)
    scale = torch.stack((xg.abs().sum((1, 3)), (xg * xg).sum((1, 3))), -1)
    n = S * (C // G)
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))             # two-pass: no cancellation
    rstd = (var + GN_EPS).rsqrt()
    y = ((xg - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(GN_B, S, C) * gamma.double() + beta.double()
    yb = y.float().to(BF)
    a64 = rstd.repeat_interleave(C // G, 1) * gamma.double()
    mag = (x.double() * a64[:, None, :]).abs() + (beta.double() - mean.repeat_interleave(C // G, 1) * a64).abs()[:, None, :]
    return dict(mag=mag, C=C, G=G, S=S, n=n, x=x, gamma=gamma, beta=beta, sums=sums, scale=scale, mean=mean, var=var, rstd=rstd,
                y=yb, ys=(yb.double() * torch.sigmoid(yb.double())).float().to(BF))


def gn_apply_f32(c, silu: bool) -> torch.Tensor:
    """the control: the kernel's expressions in f32 from the exact sums -- rstd = rsqrt(f32(var) + eps), a = rstd gamma,
    d = beta - f32(mean) a, y = bf16(x a + d), out = bf16(y / (1 + 2^(-y log2 e)))"""
    mean = c["sums"][..., 0] / c["n"]
    var = (c["sums"][..., 1] / c["n"] - mean * mean).clamp_min(0)
    rstd = (var.float() + torch.tensor(GN_EPS, dtype=torch.float32)).rsqrt()
    cpg = c["C"] // c["G"]
    a = rstd.repeat_interleave(cpg, 1) * c["gamma"]
    d = c["beta"] - mean.float().repeat_interleave(cpg, 1) * a
    y = (c["x"].float() * a[:, None, :] + d[:, None, :]).to(BF)
    if not silu:
        return y
    yf = y.float()
    return (yf * torch.reciprocal(1.0 + torch.exp2(yf * torch.tensor(-1.4426950408889634)))).to(BF)


def bf16_steps(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """distance in bf16 steps between two bf16 tensors (ordinals of the sign-magnitude encoding)"""
    def ordinal(t):
        i = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        return torch.where(i >= 0x8000, 0x8000 - i, i)
    return (ordinal(a) - ordinal(b)).abs()


def bf16_step(t: torch.Tensor) -> torch.Tensor:
    """the bf16 spacing at |t| (f64)"""
    return torch.exp2(torch.floor(torch.log2(t.double().abs().clamp_min(2.0 ** -126))) - 7)


def check_gn_apply(got: torch.Tensor, c, silu: bool, what: str = ""):
    """against the f64 statement rounded at the two rounding points -> (elements that differ at all, total).  Allowed: one bf16 step
    at each rounding point.  Without SiLU that is one step of the output.  With it, a y that rounded the other way (one step of y)
    goes through the SiLU (slope at most 1.1; its output can sit a binade lower, where steps are half as wide) and the output may
    round the other way once more: 1.1 step(y) + step(out).  Where x a and d cancel, the f32 error of the two terms exceeds a step of
    the tiny result: 2^-21 (|x a| + |d|) on top (a and d carry four and six f32 roundings)."""
    want = c["ys"] if silu else c["y"]
    g, w = got.cpu().double(), want.double()
    allowed = bf16_step(w) + (1.1 * bf16_step(c["y"]) if silu else 0.0) + 2.0 ** -21 * c["mag"]
    ok = (g - w).abs() <= allowed
    assert bool(torch.isfinite(g).all()) and bool(ok.all()), f"{what}C {c['C']} G {c['G']} S {c['S']}: {int((~ok).sum())} elements off"
    return int((g != w).sum()), g.numel()


def check_gn_stats(sums: torch.Tensor, c, what: str = "") -> float:
    """(sum, sum of squares) against f64 within STATS_REL of their cancellation-free magnitude"""
    ratio = float(((sums.double().cpu() - c["sums"]).abs() / (STATS_REL * c["scale"] + 1e-9)).max())
    print(f"{what}gn_stats C {c['C']} G {c['G']} S {c['S']}: err/tol {ratio:.3f}")
    assert ratio <= 1.0
    return ratio


def gn_rstd_error(sums: torch.Tensor, c) -> float:
    """relative error of the rstd a consumer derives from `sums` (var = E[x^2] - mean^2) against the f64 two-pass rstd"""
    s = sums.double().cpu()
    mean = s[..., 0] / c["n"]
    var = (s[..., 1] / c["n"] - mean * mean).clamp_min(0)
    return float((((var + GN_EPS).rsqrt() - c["rstd"]) / c["rstd"]).abs().max())


def gn_stats_f32(c, rows_per_thread: int = 64) -> torch.Tensor:
    """the control of the statistics: f32 partial sums of x and x^2 over runs of rows (one thread's share), f64 across the runs"""
    xg = c["x"].float()
    B, S, C = xg.shape
    pad = (-S) % rows_per_thread
    xp = torch.cat((xg, torch.zeros(B, pad, C)), 1).reshape(B, -1, rows_per_thread, C)
    s1 = torch.zeros(B, xp.shape[1], C)
    s2 = torch.zeros(B, xp.shape[1], C)
    for r in range(rows_per_thread):            # sequential f32 accumulation, as a thread does
        s1 = s1 + xp[:, :, r]
        s2 = s2 + xp[:, :, r] * xp[:, :, r]
    cpg = C // c["G"]
    return torch.stack((s1.double().sum(1).reshape(B, c["G"], cpg).sum(-1), s2.double().sum(1).reshape(B, c["G"], cpg).sum(-1)), -1)


def check_gn_table(table: torch.Tensor, c) -> float:
    """[B, C / 8, 16] against the f64 a = rstd gamma, d = beta - mean a: four f32 roundings (rsqrt, the cast of var, two products)
    on a, two more on d -> 4 x 2^-24 |a| and 2^-23 (|beta| + 2 |mean a|)"""
    B, C = GN_B, c["C"]
    cpg = C // c["G"]
    a64 = c["rstd"].repeat_interleave(cpg, 1) * c["gamma"].double()
    m = c["mean"].repeat_interleave(cpg, 1)
    d64 = c["beta"].double() - m * a64
    t = table.double().cpu()
    a, d = t[:, :, :8].reshape(B, C), t[:, :, 8:].reshape(B, C)
    ra = float(((a - a64).abs() / (2.0 ** -22 * a64.abs())).max())
    rd = float(((d - d64).abs() / (2.0 ** -23 * (c["beta"].double().abs() + 2 * (m * a64).abs()) + 1e-30)).max())
    print(f"gn_table C {C} G {c['G']} S {c['S']}: err/tol a {ra:.3f}, d {rd:.3f}")
    assert ra <= 1.0 and rd <= 1.0
    return max(ra, rd)


# ============================================================================================= attention_hd512
# (T, keys per frame, masked, key-split workspace).  Every case carries selector rows: a query whose q is a multiple of one key, so
# that key holds nearly all its weight, with that key's V made large (HD_VBIG) -- a key wrongly dropped, or a masked key wrongly
# admitted, moves the output by far more than any tolerance.
HD_C = 512
HD_VBIG = 64.0
HD_CASES = [("3x64", 3, 64, True, False), ("2x37", 2, 37, True, False), ("2x37_nomask", 2, 37, False, False),
            ("4x1024_split", 4, 1024, True, True)]
HD_SCALE = 4.0 * HD_C ** -0.5


@functools.lru_cache(maxsize=2)
def hd_case(name: str):
    _, T, hw, masked, split = next(c for c in HD_CASES if c[0] == name)
    S = T * hw
    q = rnd(f"hd.q.{name}", (1, S, HD_C), seed=331).float()
    k = rnd(f"hd.k.{name}", (1, S, HD_C), seed=332).float()
    v = rnd(f"hd.v.{name}", (1, S, HD_C), seed=333).float()
    bias = rnd(f"hd.b.{name}", (HD_C,), std=0.1, seed=334, dtype=torch.float32)
    last = S - hw                          # first row of the last frame: sees every key
    # (query row, selected key): keys 0, 31, 32, S - 1 from rows of the last frame; the last key of the query's own frame and the
    # first key of the NEXT frame (masked: invisible) from rows of frame 0
    sel = [(last + 1, 0), (last + 2, 31), (last + 3, 32 % S), (S - 1, S - 1), (S - 2, S - 1), (0, hw - 1), (hw - 1, hw - 1),
           (1, hw), (hw - 2, hw)]
    for i, j in sel:
        q[0, i] = (k[0, j] * (40.0 / (HD_SCALE * float((k[0, j] ** 2).sum())))).to(BF).float()    # score ~ 40 nats above the rest
        # (the first key of frame 1 gets 8 x that: larger than anything a frame-0 row can legitimately hold)
        v[0, j] = (8.0 if j == hw else 1.0) * HD_VBIG * (1.0 + 0.01 * torch.arange(HD_C) / HD_C)
    return dict(name=name, T=T, hw=hw, S=S, masked=masked, split=split, q=q.to(BF), k=k.to(BF), v=v.to(BF), bias=bias, sel=sel)


def hd_visible(S: int, hw: int, masked: bool, shift: int = 0) -> torch.Tensor:
    """[S query, S key] visibility: key frame <= query frame (unet_causal_3d_blocks.py:52-60).  shift: the mutant's key offset"""
    if not masked:
        return torch.ones(S, S, dtype=torch.bool)
    i = torch.arange(S)
    return ((i[None, :] - shift).clamp_min(0) // hw) <= (i[:, None] // hw)


def hd_reference(c):
    """f64 softmax(q k^T scale + mask) v + bias and the derived tolerance.  The kernel rounds P = 2^(s - M) to bf16 (nearest even:
    |d_i| <= 2^-9) for the P.V product and divides by the f32 sum of the UNROUNDED P, so out_j - ref_j = sum_i p_i d_i v_ij:
    tol_j = C_BF16 EPS_BF16 sum_i p_i |v_ij| + 2^-8 |ref_j|  (tests/cpu_ops_attn_f64.py's constants: C = 2 covers v_exp_f32 and the
    f32 score sums; 2^-8 |ref_j| is the one rounding of the output).  No absolute floor."""
    from tests import cpu_ops_attn_f64 as AF
    q, k, v = c["q"][0].double(), c["k"][0].double(), c["v"][0].double()
    s = (q @ k.T) * HD_SCALE
    s = s.masked_fill(~hd_visible(c["S"], c["hw"], c["masked"]), float("-inf"))
    p = torch.softmax(s, -1)
    ref = p @ v + c["bias"].double()
    tol = AF.C_BF16 * AF.EPS_BF16 * (p @ v.abs()) + 2.0 ** -8 * ref.abs()
    return ref, tol


def hd_control(c, mutant: str = "") -> torch.Tensor:
    """the kernel in torch: f32 scores, P rounded to bf16 for P.V, f32 sum of the unrounded P, bias, one rounding.  Mutants: key 31
    dropped; the frame mask shifted by one key."""
    q, k, v = c["q"][0].float(), c["k"][0].float(), c["v"][0].float()
    s = (q @ k.T) * torch.tensor(HD_SCALE * 1.4426950408889634, dtype=torch.float32)
    vis = hd_visible(c["S"], c["hw"], c["masked"], 1 if mutant == "mask_shift" else 0)
    if mutant == "key_dropped":
        vis = vis.clone()
        vis[:, 31] = False
    s = s.masked_fill(~vis, -1e30)
    e = torch.exp2(s - s.amax(-1, keepdim=True))
    e = torch.where(vis, e, torch.zeros_like(e))
    return ((e.to(BF).float() @ v) / e.sum(-1, keepdim=True) + c["bias"]).to(BF)


def check_hd(got: torch.Tensor, c, ref_tol=None, what: str = "") -> float:
    ref, tol = ref_tol or hd_reference(c)
    g = got.double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(g).all())
    ratio = float(((g - ref).abs() / tol).max())
    rows = sorted({i for i, _ in c["sel"]})
    rsel = float(((g - ref).abs() / tol)[rows].max())
    print(f"{what}hd512 {c['name']}: err/tol {ratio:.3f} (selector rows {rsel:.3f})")
    assert ratio <= 1.0, f"hd512 {c['name']}: err/tol {ratio:.3f}"
    if c["masked"]:      # rows of frame 0 selecting the first key of frame 1: that key's V must not be in the output at all
        for i, j in c["sel"]:
            if j // c["hw"] > i // c["hw"]:
                assert float(g[i].abs().max()) < 2 * HD_VBIG, f"row {i} contains the V of masked key {j}"
    return ratio
