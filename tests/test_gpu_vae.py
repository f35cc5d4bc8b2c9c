"""GPU parity tests of the causal 3-D VAE path: kernels (through the C ABI) against the CPU oracle, then the whole
encode / decode against the goldens produced by the real reference, then size-independent properties at the
BASELINE config-3 size (33 x 256 x 256)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import configs, synth, vae_oracle as V
from tests.util import assert_parity, finite_retry, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rnd(name, shape, std=1.0, seed=11):
    return torch.from_numpy(synth.bf16_round(synth.normal(name, seed, shape, std=std)))


def _pack_w(w, cin_p):
    """[Cout, Cin, k, k, k] fp32 (bf16-representable) -> the kernel's [Cout, Kpad] bf16 layout."""
    co, ci, k = w.shape[0], w.shape[1], w.shape[2]
    wk = torch.zeros(co, k, k, k, cin_p)
    wk[..., :ci] = w.permute(0, 2, 3, 4, 1)
    K = k ** 3 * cin_p
    out = torch.zeros(co, (K + 63) // 64 * 64)
    out[:, :K] = wk.reshape(co, K)
    return out.to(DEV).to(BF)


def _conv_ref(x, w, b, stride, up, res):
    """x NCTHW fp32 -> NCTHW fp64 reference of upsample -> replicate/causal pad -> conv (+res)."""
    k = w.shape[-1]
    xs = x.double()
    if up[0] or up[1]:
        xs = V.upsample_nearest_causal(xs, (2 if up[0] else 1, 2 if up[1] else 1, 2 if up[1] else 1))
    if k > 1:
        xs = F.pad(xs, (k // 2, k // 2, k // 2, k // 2, k - 1, 0), mode="replicate")
    y = F.conv3d(xs, w.double(), b.double(), stride=stride)
    return y if res is None else y + res.double()


CONV_CASES = [
    # Cin, Cout, k, stride, up(t, hw), B, T, H, W, residual
    (3, 32, 3, (1, 1, 1), (False, False), 1, 5, 12, 10, False),      # encoder conv_in (3 -> 8 padded channels)
    (32, 64, 3, (1, 1, 1), (False, False), 2, 3, 9, 7, True),        # Cin < 64 path, ragged M, residual
    (64, 64, 3, (1, 2, 2), (False, False), 1, 4, 11, 13, False),     # spatial downsample, odd H/W
    (64, 128, 3, (2, 2, 2), (False, False), 1, 5, 8, 8, False),      # spatio-temporal downsample
    (128, 128, 3, (1, 1, 1), (True, True), 1, 3, 6, 5, False),       # upsample T,H,W folded into the gather
    (64, 64, 3, (1, 1, 1), (False, True), 2, 2, 5, 6, False),        # upsample H,W only
    (128, 128, 3, (1, 1, 1), (True, True), 1, 1, 4, 4, False),       # single frame: T_out = 1
    (128, 3, 3, (1, 1, 1), (False, False), 1, 3, 10, 9, False),      # decoder conv_out (3 channels, scalar stores)
    (16, 128, 3, (1, 1, 1), (False, False), 1, 3, 6, 6, False),      # decoder conv_in
    (32, 32, 1, (1, 1, 1), (False, False), 1, 3, 5, 7, False),       # quant_conv (K = 32 padded to 64)
    (64, 128, 1, (1, 1, 1), (False, False), 1, 2, 9, 9, False),      # conv_shortcut
    (256, 160, 3, (1, 1, 1), (False, False), 1, 2, 6, 7, True),      # two N tiles, ragged N
    (512, 512, 3, (1, 1, 1), (False, False), 1, 2, 4, 4, True),      # widest layer
    # >= 256 output voxels, Cin % 128 == 0, Cout >= 128: the large-tile kernel with the asm K segments (conv3d_256.hip)
    (128, 256, 3, (1, 2, 2), (False, False), 2, 3, 20, 18, True),    # 2 batches, spatial stride, residual, 256-wide tile
    (256, 160, 3, (1, 1, 1), (False, False), 1, 3, 10, 11, True),    # 128-wide tile, ragged N (160) and ragged M (330)
    (128, 128, 1, (1, 1, 1), (False, False), 1, 4, 9, 9, False),     # 1x1x1: a single K segment of 2 steps
    (512, 512, 3, (2, 2, 2), (False, False), 1, 5, 24, 24, True),    # spatio-temporal stride, 8 K steps per tap
    (256, 256, 3, (1, 1, 1), (True, True), 1, 2, 7, 9, False),       # upsample T,H,W folded into the gather
    (128, 384, 3, (1, 1, 1), (False, True), 1, 2, 8, 8, False),      # H,W upsample only, ragged N: whole 16 x 16 bricks -> convsw_kernel<8, UP>
    # Cout <= 4, Cin == 128, W % 64 == 0: the reduction kernel of the decoder's conv_out (conv_fewout_kernel, v_dot2_f32_bf16)
    (128, 3, 3, (1, 1, 1), (False, False), 2, 3, 6, 64, False),      # two batch items, every row clamps at both ends
    (128, 4, 3, (1, 1, 1), (False, False), 1, 2, 5, 128, True),      # 4 output channels, residual, two segments per row
    # stride 1, no upsample, whole 16 x 16 bricks, Cin % 128 == 0: the sliding-window kernel (convsw_kernel, halo brick in LDS)
    (128, 128, 3, (1, 1, 1), (False, False), 1, 3, 32, 48, True),    # Cout == 128: two-frame tiles, odd T (the last pair has one frame), all brick kinds
    (256, 256, 3, (1, 1, 1), (False, False), 2, 2, 16, 32, False),   # 256-wide tile, two batch items, 4 body iterations
    (128, 384, 3, (1, 1, 1), (False, False), 1, 4, 16, 16, True),    # one brick per frame (every side clamps), ragged N (256 + 128)
    (512, 128, 3, (1, 1, 1), (False, False), 1, 1, 16, 16, False),   # single frame (one-frame 128-wide form): all three slots hold frame 0
    (128, 192, 3, (1, 1, 1), (False, False), 1, 2, 16, 16, False),   # 128 < Cout < 256: the one-frame 128-wide form, ragged second N tile
    (256, 128, 3, (1, 1, 1), (False, False), 2, 4, 16, 16, True),    # Cout == 128: the two-frame form (convsw2_kernel), even T, two batch items
    # the same kernel with the decoder's upsample folded into the halo (10 x 10 source patch per frame slot)
    (256, 256, 3, (1, 1, 1), (True, True), 1, 2, 8, 16, False),      # T, H, W upsample: 3 output frames of 16 x 32
    (128, 128, 3, (1, 1, 1), (False, True), 2, 2, 16, 8, True),      # H, W only, 128-wide tile, residual, two batch items
    (512, 384, 3, (1, 1, 1), (True, True), 1, 3, 8, 8, True),        # 5 output frames, ragged N (256 + 128), 8 iterations
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: f"{c[0]}to{c[1]}k{c[2]}s{''.join(map(str, c[3]))}u{int(c[4][0])}{int(c[4][1])}")
def test_causal_conv3d(hip_lib, case):
    ci, co, k, stride, up, B, T, H, W, with_res = case
    x = rnd("x", (B, ci, T, H, W))
    w = rnd("w", (co, ci, k, k, k), std=(ci * k ** 3) ** -0.5)
    b = rnd("b", (co,), std=0.1)
    cip = 8
    while cip < ci:
        cip *= 2
    xn = torch.zeros(B, T, H, W, cip)
    xn[..., :ci] = x.permute(0, 2, 3, 4, 1)
    To, Ho, Wo = hip_lib.conv_out_dims(T, H, W, stride, up)
    res = rnd("res", (B, co, To, Ho, Wo)) if with_res else None
    ref = _conv_ref(x, w, b, stride, up, res)
    assert tuple(ref.shape[2:]) == (To, Ho, Wo)
    out = torch.full((B, To, Ho, Wo, co), float("nan"), dtype=BF, device=DEV)
    hip_lib.causal_conv3d(xn.to(DEV).to(BF), _pack_w(w, cip), b.to(DEV).float(), out, k, stride, up,
                          None if res is None else res.permute(0, 2, 3, 4, 1).contiguous().to(DEV).to(BF))
    got = out.float().cpu().permute(0, 4, 1, 2, 3).double()
    # f32 accumulation of exact bf16 products + one bf16 rounding
    err = (got - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 1e-3 * float(ref.abs().max())
    assert torch.isfinite(got).all() and (err <= tol).all(), f"max err {err.max():.3e} (ref max {ref.abs().max():.3e})"

GN_FUSED_CASES = [
    # Cin, Cout, k, stride, up, B, T, H, W, residual, G, expect_fused
    (128, 128, 3, (1, 1, 1), (False, False), 1, 3, 20, 18, True, 32, True),    # 128-wide 8-wave tile, 4 channels per group, ragged M
    (128, 256, 3, (1, 2, 2), (False, False), 2, 2, 32, 32, True, 32, True),    # 4-wave tile, 8 per group, 2 batch items (256 | To Ho Wo)
    (256, 512, 3, (1, 1, 1), (True, True), 1, 2, 7, 9, False, 32, True),       # 16 per group, upsample folded in, two N tiles
    (128, 384, 1, (1, 1, 1), (False, False), 1, 4, 9, 9, False, 48, True),     # ragged N for the 256-wide tile (256 + 128), 8 per group
    (128, 256, 3, (1, 1, 1), (False, False), 2, 3, 10, 11, False, 32, False),  # a 256-voxel tile would straddle the batch items
    (64, 128, 3, (1, 1, 1), (False, False), 1, 3, 12, 12, False, 32, False),   # Cin % 128 != 0: small-tile kernel, no fused epilogue
    (128, 160, 3, (1, 1, 1), (False, False), 1, 3, 12, 12, False, 32, False),  # 5 channels per group
    (128, 128, 3, (1, 1, 1), (False, False), 1, 3, 32, 16, True, 32, True),    # sliding-window kernel, 128-wide, 4 per group
    (256, 512, 3, (1, 1, 1), (False, False), 2, 2, 16, 16, False, 32, True),   # sliding-window kernel, 256-wide, two batch items
    (128, 256, 3, (1, 1, 1), (True, True), 1, 2, 8, 8, False, 32, True),       # sliding-window kernel, upsample folded in
]


@pytest.mark.parametrize("case", GN_FUSED_CASES, ids=lambda c: f"{c[0]}to{c[1]}k{c[2]}B{c[5]}G{c[10]}")
def test_conv_fused_groupnorm_statistics(hip_lib, case):
    """osk_causal_conv3d_gn_ndhwc_bf16: same output bits as the plain conv, and gn_sums == the statistics of that output
    (f64 sums of the bf16 values; the kernel's per-tile partials are f32: relative 1e-5); shapes the fused epilogue does
    not take report fused = False, leave gn_sums untouched and still run the conv."""
    ci, co, k, stride, up, B, T, H, W, with_res, G, expect = case
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(B, T, H, W, ci, generator=g, device=DEV).to(BF)
    w = _pack_w(torch.randn(co, ci, k, k, k, generator=g, device=DEV).cpu() * (ci * k ** 3) ** -0.5, ci)
    b = (torch.randn(co, generator=g, device=DEV) * 0.1 + 0.3).float()
    To, Ho, Wo = hip_lib.conv_out_dims(T, H, W, stride, up)
    res = torch.randn(B, To, Ho, Wo, co, generator=g, device=DEV).to(BF) if with_res else None
    plain = torch.empty(B, To, Ho, Wo, co, dtype=BF, device=DEV)
    hip_lib.causal_conv3d(x, w, b, plain, k, stride, up, res)
    out = torch.full_like(plain, float("nan"))
    sums = torch.zeros(B, G, 2, dtype=torch.float64, device=DEV)
    out2, fused = hip_lib.causal_conv3d(x, w, b, out, k, stride, up, res, gn_sums=sums)
    assert fused == expect
    assert torch.equal(out2.view(torch.int16), plain.view(torch.int16))
    if not fused:
        assert float(sums.abs().sum()) == 0.0
        return
    xf = plain.double().reshape(B, -1, G, co // G)
    exact = torch.stack((xf.sum((1, 3)), (xf * xf).sum((1, 3))), -1)
    n = xf.shape[1] * xf.shape[3]
    scale = torch.stack((xf.abs().sum((1, 3)), (xf * xf).sum((1, 3))), -1)      # cancellation-free magnitude of each sum
    assert ((sums - exact).abs() <= 2e-5 * scale + 1e-9).all(), ((sums - exact).abs() / scale).max()
    if co & (co - 1) == 0:     # the stand-alone statistics kernel (power-of-two channel counts) agrees
        ref = torch.zeros_like(sums)
        hip_lib.groupnorm_stats(plain, G, ref)
        assert ((ref - exact).abs() <= 2e-5 * scale + 1e-9).all()
    # what the consumer computes from it: mean and rstd of every (batch, group)
    mean, mean_x = sums[..., 0] / n, exact[..., 0] / n
    var, var_x = sums[..., 1] / n - mean ** 2, exact[..., 1] / n - mean_x ** 2
    assert torch.allclose(mean, mean_x, rtol=0, atol=2e-5 * float(plain.float().abs().max()))
    assert torch.allclose(var, var_x, rtol=1e-4, atol=1e-6)


GN_IN_CASES = [
    # Cin, Cout, B, T, H, W, residual, G of the OUTPUT statistics (0 = none)      kernel
    (128, 128, 1, 4, 32, 32, False, 32),     # convsw2_kernel<GN>: two body iterations, fused output statistics
    (256, 128, 1, 5, 32, 48, True, 0),       # convsw2_kernel<GN>: odd T (the last pair's second frame does not exist), residual
    (128, 256, 2, 3, 32, 32, True, 32),      # convsw_kernel<8, false, GN>: batch 2 (one table per item), residual + statistics
    (256, 512, 1, 2, 16, 32, False, 0),      # two 256-channel tiles per brick, a single brick row (both H borders in one halo)
    (512, 512, 1, 3, 16, 16, False, 32),     # eight channel-block pairs: the table pointer walks 16 blocks
    (128, 320, 1, 2, 32, 16, False, 0),      # ragged last channel tile (64 of 256)
]


@pytest.mark.parametrize("case", GN_IN_CASES, ids=lambda c: f"{c[0]}to{c[1]}B{c[2]}T{c[3]}")
def test_conv_with_the_input_groupnorm_folded_in(hip_lib, case):
    """osk_causal_conv3d_gnin_ndhwc_bf16 (norm -> SiLU -> conv of ResnetBlockCausal3D, unet_causal_3d_blocks.py:247-256, with the
    normalised tensor never written): (1) against the two-launch path it replaces -- osk_groupnorm_apply_ndhwc_bf16 then the plain
    conv -- the conv INPUTS are produced with the same instructions and rounding points, so the outputs may differ only through
    the f32 accumulation order: <= 2^-7 of the output scale element-wise and relL2 <= 2e-3; (2) against the fp64 evaluation of
    conv(silu(GroupNorm(x))) under the usual parity bound; (3) the fused OUTPUT statistics against a stats pass over the result."""
    ci, co, B, T, H, W, use_res, G_out = case
    g = torch.Generator(device=DEV).manual_seed(ci + co + T)
    x = (torch.randn(B, T, H, W, ci, device=DEV, generator=g) * 1.7 + 0.4).to(BF)
    w = (torch.randn(co, 27 * ci, device=DEV, generator=g) * (27 * ci) ** -0.5).to(BF)
    b = torch.randn(co, device=DEV, generator=g) * 0.1
    gamma = 1.0 + 0.3 * torch.randn(ci, device=DEV, generator=g)
    beta = 0.2 * torch.randn(ci, device=DEV, generator=g)
    res = torch.randn(B, T, H, W, co, device=DEV, generator=g).to(BF) if use_res else None
    G = 32
    sums = torch.empty(B, G, 2, dtype=torch.float64, device=DEV)
    hip_lib.groupnorm_stats(x, G, sums)
    # the path being replaced
    h = hip_lib.groupnorm_apply(x, sums, gamma, beta, torch.empty_like(x), G, 1e-6, True)
    want = hip_lib.causal_conv3d(h, w, b, torch.empty(B, T, H, W, co, dtype=BF, device=DEV), 3, res=res)
    # the folded path
    table = hip_lib.groupnorm_table(sums, gamma, beta, torch.empty(B, ci // 8, 16, device=DEV), T * H * W, G, 1e-6)
    got = torch.full((B, T, H, W, co), float("nan"), dtype=BF, device=DEV)
    osum = torch.zeros(B, G_out, 2, dtype=torch.float64, device=DEV) if G_out else None
    ran, fused = hip_lib.causal_conv3d_gn_in(x, table, w, b, got, 3, res=res, gn_sums=osum)
    torch.cuda.synchronize()
    assert ran and fused == bool(G_out)
    assert torch.isfinite(got.float()).all()
    d = (got.float() - want.float()).abs().max().item()
    assert d <= 2.0 ** -7 * want.float().abs().max().item(), d
    assert rel_l2(got.float().cpu(), want.float().cpu()) <= 2e-3
    # fp64 reference of the whole chain
    xf = x.double().cpu()
    n = T * H * W * (ci // G)
    xg = xf.reshape(B, -1, G, ci // G)
    mean = xg.mean((1, 3))
    var = (xg * xg).mean((1, 3)) - mean * mean
    rstd = (var + 1e-6).rsqrt()
    y = (xg - mean[:, None, :, None]) * rstd[:, None, :, None]
    y = y.reshape(B, T, H, W, ci) * gamma.double().cpu() + beta.double().cpu()
    y = y * torch.sigmoid(y)
    wk = w.double().cpu().reshape(co, 3, 3, 3, ci).permute(0, 4, 1, 2, 3)
    ref = _conv_ref(y.permute(0, 4, 1, 2, 3), wk, b.cpu(), (1, 1, 1), (False, False),
                    None if res is None else res.cpu().permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1)
    assert_parity(got, ref, want, "conv(silu(gn(x))) folded into the conv (comparator: apply + conv)")
    if G_out:
        chk = hip_lib.groupnorm_stats(got, G_out, torch.empty_like(osum))
        assert torch.allclose(osum, chk, rtol=1e-5, atol=1e-2), (osum - chk).abs().max()


def test_conv_with_folded_groupnorm_declines_other_shapes(hip_lib):
    """shapes the sliding-window GN kernels do not take: ran is False and NOTHING is launched (the output keeps its sentinel) --
    hunyuan_vae._gn_silu_conv then runs apply + conv"""
    for (ci, co, T, H, W) in [(128, 128, 1, 32, 32),      # Cout == 128 needs frame pairs
                              (128, 256, 2, 24, 32),      # H is not whole 16-row bricks
                              (64, 256, 2, 16, 16)]:      # Cin % 128
        x = torch.randn(1, T, H, W, ci, device=DEV).to(BF)
        w = torch.randn(co, 27 * ci, device=DEV).to(BF)
        table = torch.ones(1, ci // 8, 16, device=DEV)
        out = torch.full((1, T, H, W, co), 7.0, dtype=BF, device=DEV)
        assert hip_lib.causal_conv3d_gn_in(x, table, w, None, out, 3) == (False, False)
        torch.cuda.synchronize()
        assert (out == 7.0).all()


def test_groupnorm_table_matches_the_apply_kernels_constants(hip_lib):
    """osk_groupnorm_table_f32: y = x a + d with the table's constants IS groupnorm_apply's y (same f32 expressions)"""
    B, S, C, G = 2, 777, 256, 32
    x = (torch.randn(B, S, C, device=DEV) * 2 + 1).to(BF)
    gamma, beta = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    sums = hip_lib.groupnorm_stats(x, G, torch.empty(B, G, 2, dtype=torch.float64, device=DEV))
    table = hip_lib.groupnorm_table(sums, gamma, beta, torch.empty(B, C // 8, 16, device=DEV), S, G, 1e-6)
    a = table[:, :, :8].reshape(B, 1, C)
    d = table[:, :, 8:].reshape(B, 1, C)
    want = hip_lib.groupnorm_apply(x, sums, gamma, beta, torch.empty_like(x), G, 1e-6, False)
    got = torch.addcmul(d, x.float(), a).to(BF)          # (torch may or may not contract to an fma: one bf16 ulp at most)
    assert (got.float() - want.float()).abs().max() <= 2.0 ** -7 * want.float().abs().max()
    assert (got != want).float().mean() < 1e-3


def test_conv3d_rejects_bad_arguments(hip_lib):
    x = torch.zeros(1, 2, 4, 4, 24, dtype=BF, device=DEV)
    w = torch.zeros(8, 27 * 24 + 8, dtype=BF, device=DEV)
    out = torch.zeros(1, 2, 4, 4, 8, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError):  # Cin not 8 * 2^j
        hip_lib.causal_conv3d(x, w, None, out, 3)
    x = torch.zeros(1, 2, 4, 4, 32, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError):  # weight rows not padded to a multiple of 64 of K = 27 * 32
        hip_lib.causal_conv3d(x, torch.zeros(8, 27 * 32, dtype=BF, device=DEV)[:, :800], None, out, 3)


@pytest.mark.parametrize("C,S,B,silu", [(32, 1000, 2, True), (64, 777, 1, True), (128, 4096, 1, False),
                                        (256, 513, 2, True), (512, 2048, 1, True)])
def test_groupnorm_silu(hip_lib, C, S, B, silu):
    x = rnd("x", (B, S, C), std=1.5) + 0.7
    x = torch.from_numpy(synth.bf16_round(x.numpy()))
    gamma, beta = rnd("g", (C,), std=0.2) + 1.0, rnd("b", (C,), std=0.2)
    xd = x.to(DEV).to(BF)
    sums = torch.empty(B, 32, 2, dtype=torch.float64, device=DEV)
    hip_lib.groupnorm_stats(xd, 32, sums)
    xg = x.double().reshape(B, S, 32, C // 32)
    assert torch.allclose(sums[:, :, 0].cpu(), xg.sum((1, 3)), rtol=1e-5, atol=1e-3)  # f32 per-thread partials, f64 across blocks
    assert torch.allclose(sums[:, :, 1].cpu(), (xg * xg).sum((1, 3)), rtol=1e-5, atol=1e-3)  # f32 per-thread partials, f64 across blocks
    out = torch.empty_like(xd)
    hip_lib.groupnorm_apply(xd, sums, gamma.to(DEV), beta.to(DEV), out, 32, 1e-6, silu)
    y = F.group_norm(x.transpose(1, 2), 32, gamma, beta, 1e-6).transpose(1, 2).to(BF).float()
    ref = (F.silu(y) if silu else y).to(BF).float()
    d = (out.float().cpu() - ref).abs()
    assert (d <= 2.0 ** -6 * ref.abs() + 2e-3).all(), f"max err {d.max():.3e}"


@pytest.mark.parametrize("S,n_hw", [(48, 16), (300, 100), (257, 0)])
def test_masked_softmax(hip_lib, S, n_hw):
    s = torch.from_numpy(synth.normal("s", 3, (S, S), std=20.0))
    Sp = (S + 63) // 64 * 64
    S4 = (S + 3) // 4 * 4
    sd = torch.zeros(S, S4, device=DEV)
    sd[:, :S] = s.to(DEV)
    probs = torch.full((S, Sp), 7.0, dtype=BF, device=DEV)
    hip_lib.masked_softmax(sd, probs, S, n_hw, 0.125)
    z = s * 0.125
    if n_hw:
        f = torch.arange(S) // n_hw
        z = z.masked_fill(f[None, :] > f[:, None], float("-inf"))
    ref = torch.softmax(z, -1)
    got = probs.float().cpu()
    assert (got[:, S:] == 0).all()
    assert (got[:, :S] - ref).abs().max() <= 2.0 ** -8


def _sd(cfg, dtype=torch.float32, device="cpu"):
    return {k: torch.from_numpy(v).to(device=device, dtype=dtype) for k, v in synth.make_params(synth.vae_param_shapes(cfg), 0).items()}


def _model(cfg):
    from open_sora_amd import hunyuan_vae

    m = hunyuan_vae.CausalVAE3D_HUNYUAN(device_map=DEV, torch_dtype=BF, **cfg)
    m.load_state_dict(_sd(cfg, BF, DEV), strict=True)
    return m


@pytest.mark.parametrize("name", list(configs.VAE_GOLDEN))
def test_vae_encode_decode_vs_reference_golden(hip_lib, name):
    cfg, B, T, H, W = configs.VAE_GOLDEN[name]
    g = np.load(os.path.join(GOLDEN_DIR, f"vae_{name}.npz"))
    m = _model(cfg)
    x = torch.from_numpy(synth.vae_video(B, T, H, W))
    zin = torch.from_numpy(synth.vae_latent(B, *g["z"].shape[2:]))
    sdb = _sd(cfg, BF)
    with torch.inference_mode():
        z = m.encode(x.to(DEV).to(BF), sample_posterior=False)
        dec = m.decode(zin.to(DEV).to(BF))
        torch.cuda.synchronize()
        z_ref = finite_retry(lambda: V.encode(sdb, cfg, x.to(BF)))     # reference-precision comparator: the oracle run in bf16
        d_ref = finite_retry(lambda: V.decode(sdb, cfg, zin.to(BF)))
    assert_parity(z, torch.from_numpy(g["z"]), z_ref, f"vae encode [{name}]")
    assert_parity(dec, torch.from_numpy(g["dec"]), d_ref, f"vae decode [{name}]")


def test_plugin_targets_on_device(hip_lib):
    """VERDICT r5 missing #6: the `from_native_module` targets of open_sora_amd/vae_plugin.py (the ShardFormer replacement convention
    of /root/reference/opensora/models/hunyuan_vae/policy.py:13-48) ON THE DEVICE -- their NCTHW <-> NDHWC conversions, the
    parameter sharing of `_Adopted` and install() / uninstall() had only run on the CPU emulation.  The "native" modules here are
    this package's own encoder / decoder / CausalConv3d (the same attribute names and state-dict keys as the reference's, which is
    all the targets read): target(x) must equal the direct engine call bit for bit, a load_state_dict through the adopted module
    must reach the native one, and the golden of the reference holds through the installed targets."""
    from open_sora_amd import hunyuan_vae as hv, vae_plugin

    name = next(iter(configs.VAE_GOLDEN))
    cfg, B, T, H, W = configs.VAE_GOLDEN[name]
    g = np.load(os.path.join(GOLDEN_DIR, f"vae_{name}.npz"))
    m = _model(cfg)
    x = torch.from_numpy(synth.vae_video(B, T, H, W)).to(DEV).to(BF)
    zin = torch.from_numpy(synth.vae_latent(B, *g["z"].shape[2:])).to(DEV).to(BF)
    with torch.inference_mode():
        # whole-module targets vs the engine called directly
        enc_t = vae_plugin.HipEncoderCausal3D.from_native_module(m.encoder)
        dec_t = vae_plugin.HipDecoderCausal3D.from_native_module(m.decoder)
        assert enc_t._parameters is m.encoder._parameters and enc_t._modules is m.encoder._modules      # the SAME dicts
        h_direct = hv._to_ncthw(hv.run_encoder(m.encoder, hv._to_ndhwc(x, hv._pad8(x.shape[1]))), BF)
        h_target = enc_t(x)
        assert h_target.shape == h_direct.shape and h_target.dtype == BF and torch.equal(h_target, h_direct)
        zq = hv._to_ncthw(hv._conv(m.post_quant_conv, hv._to_ndhwc(zin, hv._pad8(zin.shape[1]))), BF)
        d_direct = hv._to_ncthw(hv.run_decoder(m.decoder, hv._to_ndhwc(zq, hv._pad8(zq.shape[1]))), BF)
        d_target = dec_t(zq)
        assert torch.equal(d_target, d_direct)
        # a float32 caller gets float32 back (the reference's fp32 VAE path), same values after rounding
        assert enc_t(x.float()).dtype == torch.float32
        # per-layer target: one CausalConv3d
        conv = m.decoder.conv_in
        c_t = vae_plugin.HipCausalConv3d.from_native_module(conv)
        c_direct = hv._to_ncthw(hv._conv(conv, hv._to_ndhwc(zq, hv._pad8(zq.shape[1]))), BF)
        assert torch.equal(c_t(zq), c_direct)
        # install on the whole autoencoder: encode / decode (its own Python around the targets) keep the reference golden
        keys = list(m.state_dict().keys())
        vae_plugin.install(m)
        assert isinstance(m.encoder, vae_plugin.HipEncoderCausal3D) and list(m.state_dict().keys()) == keys
        # the package's encode() drives run_encoder(self.encoder, ...) -- which now receives the ADOPTED module: same attributes
        z = m.encode(x, sample_posterior=False)
        dec = m.decode(zin)
        sdb = _sd(cfg, BF)
        z_ref = finite_retry(lambda: V.encode(sdb, cfg, x.cpu()))
        d_ref = finite_retry(lambda: V.decode(sdb, cfg, zin.cpu()))
        assert_parity(z, torch.from_numpy(g["z"]), z_ref, f"vae encode through installed targets [{name}]")
        assert_parity(dec, torch.from_numpy(g["dec"]), d_ref, f"vae decode through installed targets [{name}]")
        # parameter sharing: new weights loaded through the adopted module reach the kernels (plans are dropped)
        sd2 = {k: v * 0.5 for k, v in m.state_dict().items()}
        m.load_state_dict(sd2, strict=True)
        z2 = m.encode(x, sample_posterior=False)
        assert not torch.equal(z2, z)
        vae_plugin.uninstall(m)
        assert not isinstance(m.encoder, vae_plugin._Adopted)
        assert torch.equal(m.encode(x, sample_posterior=False), z2)          # the native module holds the same (new) parameters


def test_vae_tiled_vs_reference_golden(hip_lib):
    name = "c32_tiled"
    cfg, B, T, H, W = configs.VAE_TILED_GOLDEN[name]
    g = np.load(os.path.join(GOLDEN_DIR, f"vae_{name}.npz"))
    m = _model(cfg)
    m.enable_tiling()
    x = torch.from_numpy(synth.vae_video(B, T, H, W))
    zin = torch.from_numpy(synth.vae_latent(B, *g["z"].shape[2:]))
    sdb = _sd(cfg, BF)
    with torch.inference_mode():
        z = m.encode(x.to(DEV).to(BF), sample_posterior=False)
        dec = m.decode(zin.to(DEV).to(BF))
        z_ref = finite_retry(lambda: V.encode_tiled(sdb, cfg, x.to(BF)))
        d_ref = finite_retry(lambda: V.decode_tiled(sdb, cfg, zin.to(BF)))
    assert_parity(z, torch.from_numpy(g["z"]), z_ref, "vae tiled encode")
    assert_parity(dec, torch.from_numpy(g["dec"]), d_ref, "vae tiled decode")


# the eight large layer shapes of BASELINE config 3 (profiles/r03k_conv_layers.jsonl: 96 % of the VAE's conv FLOPs), each at its
# real size: (Cin, Cout, T, H, W, upsample (t, hw), kernel that takes it)
_FULL_SIZE_LAYERS = [
    (128, 128, 33, 256, 256, (False, False), "convsw2_kernel (two-frame tiles)"),
    (256, 128, 33, 256, 256, (False, False), "convsw2_kernel"),
    (256, 256, 33, 128, 128, (False, False), "convsw_kernel<8>"),
    (512, 256, 33, 128, 128, (False, False), "convsw_kernel<8>: 2112 tiles, 8.25 rounds"),
    (512, 512, 17, 64, 64, (False, False), "convsw_kernel<8>"),
    (512, 512, 9, 32, 32, (False, False), "convsw_kernel<8>, 144 tiles"),
    (512, 512, 9, 32, 32, (True, True), "convsw_kernel<8, UP>: dec.up0 upsampler -> 17 x 64 x 64"),
    (256, 256, 17, 128, 128, (True, True), "convsw_kernel<8, UP>: dec.up2 upsampler -> 33 x 256 x 256"),
    (512, 512, 17, 64, 64, (True, True), "convsw_kernel<8, UP>: dec.up1 upsampler -> 33 x 128 x 128"),
]


@pytest.mark.parametrize("ci,co,T,H,W,up,what", _FULL_SIZE_LAYERS, ids=[f"{c[0]}to{c[1]}_{c[2]}x{c[3]}{'_up' if c[5][0] else ''}" for c in _FULL_SIZE_LAYERS])
def test_full_size_conv_spot_check(hip_lib, ci, co, T, H, W, up, what):
    """BASELINE config 3 size (VERDICT r3 weak #1b): every large conv layer shape of the encode + decode at its REAL extent --
    not only the decoder's last upsampler -- checked voxel by voxel on a random sample (corners and borders included) against a
    direct fp64 evaluation of pad(upsample(x)) * w + bias, written into a NaN-filled output."""
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(1, T, H, W, ci, device=DEV, generator=g).to(BF)
    w = (torch.randn(co, 3, 3, 3, ci, device=DEV, generator=g) * (27 * ci) ** -0.5).to(BF)
    b = torch.randn(co, device=DEV, generator=g) * 0.1
    To, Ho, Wo = hip_lib.conv_out_dims(T, H, W, (1, 1, 1), up)
    out = torch.full((1, To, Ho, Wo, co), float("nan"), dtype=BF, device=DEV)
    hip_lib.causal_conv3d(x, w.reshape(co, -1).contiguous(), b, out, 3, (1, 1, 1), up)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all(), what
    rs = np.random.RandomState(ci + co + T)
    pts = [(0, 0, 0), (To - 1, Ho - 1, Wo - 1), (1, 0, Wo - 1), (2, Ho - 1, 0), (To - 1, 15, 16), (0, Ho - 16, Wo - 17)] + \
          [(rs.randint(To), rs.randint(Ho), rs.randint(Wo)) for _ in range(58)]
    xc, wc, bc = x[0].double(), w.double(), b.double()
    for (t, h, ww) in pts:
        acc = bc.clone()
        for dt in range(3):
            tu = min(max(t + dt - 2, 0), To - 1)
            ts = (0 if tu == 0 else 1 + (tu - 1) // 2) if up[0] else tu
            for dh in range(3):
                hs = min(max(h + dh - 1, 0), Ho - 1) // (2 if up[1] else 1)
                for dw in range(3):
                    ws = min(max(ww + dw - 1, 0), Wo - 1) // (2 if up[1] else 1)
                    acc += wc[:, dt, dh, dw, :] @ xc[ts, hs, ws]
        got = out[0, t, h, ww].double()
        assert (got - acc).abs().max() <= 2.0 ** -7 * acc.abs().max() + 1e-3, (what, t, h, ww)


@pytest.mark.parametrize("fold", [False, True], ids=["apply+conv", "gn_folded"])
def test_full_size_encode_decode_vs_reference_fixture(hip_lib, fold):
    """(fold: hunyuan_vae.FOLD_GN -- the opt-in path whose resnet convs read the un-normalised tensor -- meets the same bounds.)
    BASELINE config 3 END TO END at its real size against the reference itself: tests/golden/vae_fullsize_cfg3.npz holds what the
    reference's own AutoencoderKLCausal3D (fp32, CPU, run once offline by oracle/make_golden_fullsize.py) returns for
    synth.vae_video(1, 33, 256, 256) / synth.vae_latent(1, 9, 32, 32) with the synthetic shipped-width weights: the whole latent
    mean, the decoded video on an 8 x 8 pixel lattice, and per (channel, frame) first and second moments of the whole video.
    Tolerance (round 5): SURVEY 8(d)'s rule against the COMMITTED reference-precision error -- the fixture also holds e_ref_z /
    e_ref_dec = relL2 of the reference's own eager-bf16 run (bf16 parameters and activations) against its fp32 run, made by the same
    script: e_ours <= max(1.5 e_ref, 2^-8), max-abs <= 4 a_ref (measured on MI355X, round 4: latent 1.10e-2 against e_ref 1.15e-2,
    decoded lattice 1.15e-2 against 1.21e-2); the per-frame moments of the whole video within the same error scale."""
    from oracle import make_golden_fullsize as FS
    from open_sora_amd import hunyuan_vae

    g = np.load(os.path.join(GOLDEN_DIR, "vae_fullsize_cfg3.npz"))
    cfg = dict(FS.CFG)
    m = _model(cfg)
    x = torch.from_numpy(synth.vae_video(*FS.SHAPE)).to(DEV).to(BF)
    hunyuan_vae.FOLD_GN = fold
    try:
        with torch.inference_mode():
            z = m.encode(x, sample_posterior=False).float().cpu()
            zin = torch.from_numpy(synth.vae_latent(1, 9, 32, 32)).to(DEV).to(BF)
            dec = m.decode(zin).float().cpu()
    finally:
        hunyuan_vae.FOLD_GN = False
    zt = torch.from_numpy(g["z"])
    assert list(z.shape) == list(zt.shape) and torch.isfinite(z).all() and torch.isfinite(dec).all()
    ez = rel_l2(z, zt)
    got = FS.summarize_dec(dec)
    ed = rel_l2(torch.from_numpy(got["dec_s8"]), torch.from_numpy(g["dec_s8"]))
    em = float(np.abs(got["dec_mean"] - g["dec_mean"]).max())
    es = float(np.abs(got["dec_sq"] - g["dec_sq"]).max() / np.abs(g["dec_sq"]).max())
    print(f"full-size cfg 3 vs the reference fixture: latent relL2 {ez:.3e}, decoded lattice relL2 {ed:.3e}, per-frame mean |d| {em:.3e}, mean-square rel {es:.3e}")
    e_ref_z, e_ref_dec, floor = float(g["e_ref_z"]), float(g["e_ref_dec"]), 2.0 ** -8
    az = float((z.double() - zt.double()).abs().max())
    ad = float(np.abs(got["dec_s8"].astype(np.float64) - g["dec_s8"]).max())
    print(f"   reference bf16 vs fp32: latent relL2 {e_ref_z:.3e} max-abs {float(g['a_ref_z']):.3e}; decoded relL2 {e_ref_dec:.3e} max-abs {float(g['a_ref_dec']):.3e};"
          f" ours max-abs latent {az:.3e} decoded lattice {ad:.3e}")
    assert ez <= max(1.5 * e_ref_z, floor) and ed <= max(1.5 * e_ref_dec, floor), (ez, ed)
    assert az <= 4.0 * float(g["a_ref_z"]) and ad <= 4.0 * float(g["a_ref_dec"]), (az, ad)
    # moments of the WHOLE video: a frame mean off by more than the reference-precision error of an rms pixel would be a bias
    rms = float(np.sqrt(np.abs(g["dec_sq"]).max()))
    assert em <= 0.5 * e_ref_dec * rms and es <= 3.0 * e_ref_dec, (em, es)


def test_large_tile_conv_is_deterministic_under_load(hip_lib):
    """race screen for the asm K loop of conv3d_256.hip (see test_hand_scheduled_kernels_are_deterministic_under_load):
    12 runs of a conv that fills the chip for several rounds, ragged voxel tile at the end, bit-identical."""
    ci, co = 256, 384
    T, H, W = 5, 61, 67
    g = torch.Generator(device=DEV).manual_seed(9)
    x = torch.randn(1, T, H, W, ci, device=DEV, generator=g).to(BF)
    w = (torch.randn(co, 27 * ci, device=DEV, generator=g) * (27 * ci) ** -0.5).to(BF)
    b = torch.randn(co, device=DEV, generator=g) * 0.1
    outs = []
    for _ in range(12):
        o = torch.empty(1, T, H, W, co, dtype=BF, device=DEV)
        hip_lib.causal_conv3d(x, w, b, o, 3)
        outs.append(o)
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:]), "conv256x / convsw: run-to-run difference"
    assert torch.isfinite(outs[0].float()).all()


def test_full_size_encode_decode_properties(hip_lib):
    """BASELINE config 3: [1,3,33,256,256] through the shipped architecture (128/256/512/512, 2 layers per block).
    Size-independent properties: shapes, finiteness, and batch independence (every kernel treats the batch items
    separately; only the f64 GroupNorm atomics may reorder)."""
    cfg = dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2)
    m = _model(cfg)
    x = torch.from_numpy(synth.vae_video(1, 33, 256, 256)).to(DEV).to(BF)
    with torch.inference_mode():
        z = m.encode(x, sample_posterior=False)
        assert list(z.shape) == [1, 16, 9, 32, 32] and torch.isfinite(z.float()).all()
        dec = m.decode(z)
        assert list(dec.shape) == [1, 3, 33, 256, 256] and torch.isfinite(dec.float()).all()
        x2 = torch.cat((x[:, :, :5, :64, :64], x[:, :, 5:10, :64, :64]), 0)
        z2 = m.encode(x2, sample_posterior=False)
        za = m.encode(x2[:1], sample_posterior=False)
        zb = m.encode(x2[1:], sample_posterior=False)
        assert (z2 - torch.cat((za, zb))).abs().max() <= 2.0 ** -6 * z2.abs().max()


@pytest.mark.parametrize("dim,shape_a,shape_b,extent", [
    (-2, (1, 3, 5, 24, 40), (1, 3, 5, 20, 40), 8),      # blend_v (vector path: inner = W = 40)
    (-1, (2, 16, 3, 12, 10), (2, 16, 3, 12, 7), 4),     # blend_h (scalar path: inner = 1)
    (-3, (1, 4, 9, 6, 12), (1, 4, 7, 6, 12), 2),        # blend_t
    (-1, (1, 3, 2, 8, 3), (1, 3, 2, 8, 16), 8),         # extent clipped to a's width (3)
])
def test_blend_kernel_vs_reference_formula(hip_lib, dim, shape_a, shape_b, extent):
    """osk_blend_bf16 vs blend_v / blend_h / blend_t (autoencoder_kl_causal_3d.py:360-382) evaluated in f64:
    b[.., y, ..] = a[.., -e + y, ..] (1 - y/e) + b[.., y, ..] (y/e), in place, untouched outside the seam."""
    g = torch.Generator(device=DEV).manual_seed(3)
    a = torch.randn(*shape_a, device=DEV, generator=g).to(BF)
    b = torch.randn(*shape_b, device=DEV, generator=g).to(BF)
    b0 = b.clone()
    out = hip_lib.blend(a, b, extent, dim)
    assert out.data_ptr() == b.data_ptr()
    e = min(a.shape[dim], b.shape[dim], extent)
    ref = b0.double().cpu()
    a64 = a.double().cpu()
    for y in range(e):
        ia, ib = [slice(None)] * 5, [slice(None)] * 5
        ia[dim], ib[dim] = a.shape[dim] - e + y, y
        ref[tuple(ib)] = a64[tuple(ia)] * (1 - y / e) + b0.double().cpu()[tuple(ib)] * (y / e)
    err = (b.double().cpu() - ref).abs()
    assert (err <= 2.0 ** -8 * ref.abs() + 1e-6).all(), err.max()
    rest = [slice(None)] * 5
    rest[dim] = slice(e, None)
    assert torch.equal(b[tuple(rest)], b0[tuple(rest)])


@pytest.mark.parametrize("B,T,hw,masked", [(1, 3, 64, True), (2, 5, 37, True), (1, 1, 300, True), (1, 4, 96, False), (1, 9, 256, True),
                                           (1, 9, 1024, True), (2, 5, 1000, True), (1, 3, 2100, False)])
def test_attention_hd512_vs_f64(hip_lib, B, T, hw, masked):
    """osk_attention_hd512_fwd_bf16 (one head of dim 512, frame-causal) against an f64 softmax(q k^T / sqrt(512) + mask) v + b
    with the reference's mask rule (unet_causal_3d_blocks.py:52-60: key frame <= query frame); ragged S (not a multiple of
    the 32-key tile / 128-query block), batch, strided q / k views, no-mask mode."""
    S, C = T * hw, 512
    Sp = (S + 63) // 64 * 64
    g = torch.Generator(device=DEV).manual_seed(S + B)
    qk = torch.randn(B, S, 2 * C, device=DEV, generator=g).to(BF)          # q, k as column views of one buffer
    q, k = qk[:, :, :C], qk[:, :, C:]
    v = torch.randn(B, S, C, device=DEV, generator=g).to(BF)
    vt = torch.zeros(B, C, Sp, dtype=BF, device=DEV)
    vt[:, :, :S] = v.transpose(1, 2)
    bias = torch.randn(C, device=DEV, generator=g) * 0.1
    out = torch.empty(B, S, C, dtype=BF, device=DEV)
    # scores of O(1) spread so that the softmax is neither flat nor one-hot
    scale = 4.0 * C ** -0.5
    hip_lib.attention_hd512(q, k, vt, bias, out, hw if masked else 0, scale)
    s = torch.einsum("bqc,bkc->bqk", q.double(), k.double()) * scale
    if masked:
        f = torch.arange(S, device=DEV) // hw
        s = s.masked_fill(f[None, None, :] > f[None, :, None], float("-inf"))
    ref = torch.softmax(s, -1) @ v.double() + bias.double()
    err = (out.double() - ref).abs()
    tol = 2.0 ** -7 * ref.abs() + 2.0 ** -7      # P is rounded to bf16 before P.V, the output once more
    assert torch.isfinite(out.float()).all() and (err <= tol).all(), (err.max().item(), (err / tol).max().item())
    out2 = torch.empty_like(out)
    hip_lib.attention_hd512(q, k, vt, bias, out2, hw if masked else 0, scale)
    assert torch.equal(out, out2)
    # key-split launch (round 4; it engages from S >= 4096: the last three cases -- frames of 1024 tokens = BASELINE config 3's mid
    # block, frames of 1000 tokens so that 128-row query blocks span two frames and a key part can be masked out entirely for some of
    # their rows, and the unmasked mode): same result up to the f32 combination of the parts, repeatable
    ws = hip_lib.attention_hd512_workspace(B, S, DEV)
    out3 = torch.full_like(out, float("nan"))
    hip_lib.attention_hd512(q, k, vt, bias, out3, hw if masked else 0, scale, workspace=ws)
    err3 = (out3.double() - ref).abs()
    assert torch.isfinite(out3.float()).all() and (err3 <= tol).all(), (err3.max().item(), (err3 / tol).max().item())
    if S < 4096:
        assert torch.equal(out3, out)            # short chains are not split
    out4 = torch.empty_like(out)
    hip_lib.attention_hd512(q, k, vt, bias, out4, hw if masked else 0, scale, workspace=ws)
    assert torch.equal(out3, out4)
