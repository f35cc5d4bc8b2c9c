"""GPU: the Video DC-AE decoder (open_sora_amd.dc_ae, csrc/dc_ae.hip) on the MI355X.

- every new kernel against an f64 evaluation of the formula of include/osk.h on bf16-representable inputs.  One rounding to bf16
  is half an ulp (2^-9 relative); the bound is twice that plus 1e-4 of the largest output for the f32 accumulation, the bound
  tests/test_gpu_flux_ae.py uses.  The conv cases judge the zero-padded border voxels separately from the interior;
- the small-geometry decode (untiled, single frame, tiled) against the committed fixture the reference itself produced;
- the shipped-width decode on a reduced latent against the plain-torch fp32 restatement (tests/dc_ae_restatement.py);
  tolerance: tests.util.assert_parity with the restatement in bf16 (CPU, never the code under test) as the comparator."""
import os
import zlib

import numpy as np
import pytest
import torch

from tests import cpu_ops_dc_ae as E
from tests import dc_ae_restatement as R
from tests.dc_ae_audit import _judge, conv_border, dw_border
from tests.util import assert_parity, finite_retry

BF = torch.bfloat16
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dc_ae_small.npz")
TILED = dict(spatial_tile_size=128, temporal_tile_size=16, tile_overlap_factor=0.25)


@pytest.fixture()
def dc_ae(hip_lib):
    from open_sora_amd import dc_ae, mmdit

    mmdit.set_ops_for_testing(hip_lib)
    torch.cuda.set_device(0)
    return dc_ae


def _gen(name):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(name.encode()) % 100000)


def _randn(shape, g, scale=1.0):
    return (scale * torch.randn(shape, generator=g, device=DEV)).to(BF)


# (name, Cin, Cout, T, H, W (source), ksize, up_t, up_hw, res, bias, silu)
CONV_CASES = [
    ("project_in_128_1024", 128, 1024, 4, 8, 8, 3, False, False, True, True, False),
    ("up_1024_1024_thw", 1024, 1024, 2, 4, 4, 3, True, True, True, True, False),
    ("up_1024_512_thw_odd", 1024, 512, 3, 3, 5, 3, True, True, True, True, False),
    ("up_1024_512_t1", 1024, 512, 1, 4, 4, 3, False, True, True, True, False),
    ("up_512_512_hw", 512, 512, 3, 8, 8, 3, False, True, True, True, False),
    ("up_512_256_hw_odd", 512, 256, 2, 5, 7, 3, False, True, False, True, False),
    ("up_256_128_hw", 256, 128, 2, 8, 16, 3, False, True, True, True, False),
    ("res_512_silu", 512, 512, 4, 8, 16, 3, False, False, False, True, True),
    ("res_256_nobias", 256, 256, 3, 16, 16, 3, False, False, False, False, False),
    ("res_128_silu_odd", 128, 128, 5, 13, 19, 3, False, False, False, True, True),
    ("res_128_t1", 128, 128, 1, 24, 32, 3, False, False, True, True, False),
    ("project_out_128_3", 128, 3, 4, 16, 32, 3, False, False, False, True, False),
    ("project_out_128_3_odd_t1", 128, 3, 1, 9, 11, 3, False, False, False, True, False),
    ("small_32_32_up_t_only", 32, 32, 3, 6, 6, 3, True, False, True, True, False),
    ("inverted_1x1_512_4096_silu", 512, 4096, 2, 5, 7, 1, False, False, False, True, True),
    ("pointwise_1x1_32_96", 32, 96, 2, 3, 5, 1, False, False, False, False, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv3d_zp_kernel_vs_f64(dc_ae, hip_lib, case):
    name, Cin, Cout, T, H, W, k, up_t, up_hw, with_res, with_bias, silu = case
    g = _gen(name)
    conv = torch.nn.Conv3d(Cin, Cout, k, bias=with_bias).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g, device=DEV) / (Cin * k ** 3) ** 0.5)
        if with_bias:
            conv.bias.copy_(0.1 * torch.randn(Cout, generator=g, device=DEV))
    plan = dc_ae._DensePlan(conv)
    x = _randn((1, T, H, W, Cin), g)
    To, Ho, Wo = T << int(up_t), H << int(up_hw), W << int(up_hw)
    res = _randn((1, To, Ho, Wo, Cout), g) if with_res else None
    out = torch.full((1, To, Ho, Wo, Cout), float("nan"), dtype=BF, device=DEV)
    hip_lib.conv3d_zp(x, plan.w, plan.b, out, k, up_t, up_hw, silu, res)
    torch.cuda.synchronize()
    y = E.conv3d_zp_ref(x, plan.w, plan.b, k, up_t, up_hw, silu, res, dtype=torch.float64)
    _judge(name, out, y, conv_border(To, Ho, Wo, DEV))


@pytest.mark.gpu
def test_conv3d_zp_refuses_unsupported_shapes_without_launch(dc_ae, hip_lib):
    x = torch.randn(1, 2, 4, 4, 24, device=DEV).to(BF)
    w = torch.zeros(8, 27 * 24 + 8, dtype=BF, device=DEV)
    out = torch.zeros(1, 2, 4, 4, 8, dtype=BF, device=DEV)
    rc = hip_lib.lib.osk_conv3d_zp_ndhwc_bf16(x.data_ptr(), 1, 2, 4, 4, 24, w.data_ptr(), w.stride(0), None, 8, 3, 0, 0, 0, None,
                                              out.data_ptr(), hip_lib._stream())
    assert rc == hip_lib.OSK_EUNSUPPORTED                                       # Cin = 24 is not 8 * 2^j
    rc = hip_lib.lib.osk_dwconv3d_ndhwc_bf16(x.data_ptr(), 1, 2, 4, 4, 24, w.data_ptr(), None, 7, 0, out.data_ptr(), hip_lib._stream())
    assert rc == hip_lib.OSK_EUNSUPPORTED                                       # k = 7
    rc = hip_lib.lib.osk_gconv32_bf16(x.data_ptr(), 32, 24, w.data_ptr(), out.data_ptr(), hip_lib._stream())
    assert rc == hip_lib.OSK_EUNSUPPORTED                                       # C % 32
    torch.cuda.synchronize()
    assert float(out.float().abs().sum()) == 0.0


# (name, Cin, Cout, T, H, W, ft, fhw)
DUP_CASES = [
    ("project_in_128_1024", 128, 1024, 3, 5, 4, 1, 1),
    ("up_1024_1024_3d", 1024, 1024, 2, 3, 5, 2, 2),
    ("up_1024_512_3d", 1024, 512, 3, 4, 4, 2, 2),
    ("up_1024_1024_t1_2d", 1024, 1024, 1, 4, 3, 1, 2),
    ("up_1024_512_t1_2d", 1024, 512, 1, 5, 5, 1, 2),
    ("up_512_512_2d", 512, 512, 4, 6, 7, 1, 2),
    ("up_256_128_2d", 256, 128, 2, 8, 9, 1, 2),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DUP_CASES, ids=[c[0] for c in DUP_CASES])
def test_dup_shuffle_kernel_is_the_reference_shortcut(dc_ae, hip_lib, case):
    """a pure gather: bit-equal to the index formula AND to repeat_interleave + pixel shuffle as the restatement states them"""
    name, Cin, Cout, T, H, W, ft, fhw = case
    x = _randn((2, T, H, W, Cin), _gen(name))
    out = torch.full((2, T * ft, H * fhw, W * fhw, Cout), float("nan"), dtype=BF, device=DEV)
    hip_lib.dup_shuffle(x, out, ft, fhw)
    torch.cuda.synchronize()
    assert torch.equal(out, E.dup_shuffle_ref(x, Cout, ft, fhw)), name
    want = R.dup_shortcut(x.permute(0, 4, 1, 2, 3), Cout, fhw, ft == 2).permute(0, 2, 3, 4, 1)
    assert torch.equal(out, want), name


# (name, C, T, H, W, ksize, glu, bias)
DW_CASES = [
    ("glu_k3_4096", 4096, 4, 8, 8, 3, True, True),
    ("glu_k3_8192_t1", 8192, 1, 4, 5, 3, True, True),
    ("glu_k3_512_odd", 512, 3, 7, 5, 3, True, True),
    ("agg_k5_1536", 1536, 4, 8, 8, 5, False, False),
    ("agg_k5_3072_tiny", 3072, 1, 2, 2, 5, False, False),
    ("agg_k5_192_odd", 192, 5, 6, 7, 5, False, False),
    ("plain_k3_bias_64", 64, 2, 9, 3, 3, False, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DW_CASES, ids=[c[0] for c in DW_CASES])
def test_dwconv3d_kernel_vs_f64(dc_ae, hip_lib, case):
    name, C, T, H, W, k, glu, with_bias = case
    g = _gen(name)
    x = _randn((1, T, H, W, C), g)
    w = _randn((k ** 3, C), g, k ** -1.5)
    b = (0.1 * torch.randn(C, generator=g, device=DEV)) if with_bias else None
    out = torch.full((1, T, H, W, C // 2 if glu else C), float("nan"), dtype=BF, device=DEV)
    hip_lib.dwconv3d(x, w, b, out, k, glu)
    torch.cuda.synchronize()
    y = E.dwconv3d_ref(x, w, b, k, glu, dtype=torch.float64)
    _judge(name, out, y, dw_border(T, H, W, k, DEV))


@pytest.mark.gpu
@pytest.mark.parametrize("M,C", [(1, 96), (32, 1536), (777, 3072), (4096, 192)])
def test_gconv32_kernel_vs_f64(dc_ae, hip_lib, M, C):
    g = _gen(f"gconv{M}x{C}")
    x, w = _randn((M, C), g), _randn((C, 32), g, 32 ** -0.5)
    out = torch.full((M, C), float("nan"), dtype=BF, device=DEV)
    hip_lib.gconv32(x, w, out)
    torch.cuda.synchronize()
    _judge(f"gconv32 {M}x{C}", out, E.gconv32_ref(x, w, dtype=torch.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,G", [(1, 1, 2), (1, 8, 32), (2, 100, 3), (1, 777, 16), (1, 4096, 32), (1, 32768, 2)])
def test_relu_linear_attn_kernel_vs_f64(dc_ae, hip_lib, B, N, G):
    g = _gen(f"la{B}x{N}x{G}")
    qkv = _randn((B, N, G * 96), g)
    v = qkv.view(B, N, G, 96)
    v[:, ::3, :, 32:64] = -v[:, ::3, :, 32:64].abs()        # every third token: relu(k) == 0 (contributes nothing to K^T V)
    v[:, :, 0, 32:64] = -v[:, :, 0, 32:64].abs()            # group 0: relu(k) == 0 for EVERY token -> 0 / (0 + eps) == 0
    if N > 1:
        v[:, 1, :, :32] = -v[:, 1, :, :32].abs()            # token 1: relu(q) == 0 -> 0
    out = torch.full((B, N, 2 * G * 32), float("nan"), dtype=BF, device=DEV)
    hip_lib.relu_linear_attn(qkv, out[:, :, G * 32:])        # the second half of a wider tensor, as the two scales write
    torch.cuda.synchronize()
    y = E.relu_linear_attn_ref(qkv, dtype=torch.float64)
    got = out[:, :, G * 32:]
    assert torch.isnan(out[:, :, : G * 32].float()).all()    # nothing written outside the G * 32 columns
    assert float(got.view(B, N, G, 32)[:, :, 0].float().abs().max()) == 0.0
    _judge(f"relu_linear_attn B{B} N{N} G{G}", got, y)


@pytest.mark.gpu
@pytest.mark.parametrize("M,C,res,relu", [(1, 128, False, True), (513, 128, False, True), (100, 256, True, False),
                                          (4096, 512, True, False), (37, 1024, True, False), (64, 32, True, False)])
def test_rmsnorm_affine_kernel_vs_f64(dc_ae, hip_lib, M, C, res, relu):
    g = _gen(f"rms{M}x{C}")
    x = _randn((M, C), g, 3.0)
    w = 1.0 + 0.1 * torch.randn(C, generator=g, device=DEV)
    b = 0.1 * torch.randn(C, generator=g, device=DEV)
    r = _randn((M, C), g) if res else None
    out = torch.full((M, C), float("nan"), dtype=BF, device=DEV)
    hip_lib.rmsnorm_affine(x, w, b, out, 1e-5, r, relu)
    torch.cuda.synchronize()
    _judge(f"rmsnorm {M}x{C}", out, E.rmsnorm_affine_ref(x, w, b, 1e-5, r, relu, dtype=torch.float64))


# ------------------------------------------------------------------------ shapes the ABI accepts and the decoder never launches
# include/osk.h takes all of these; the bound is the one above.  Batch elements hold different data (one generator stream over
# the whole tensor), so a wrong batch index cannot cancel.
# (name, B, Cin, Cout, T, H, W (source), ksize, up_t, up_hw, res, bias, silu)
CONV_CASES_MORE = [
    # batch > 1 on the 8 x 16 brick path (Hu % 8 == 0, Wu % 16 == 0): frame = q / bh runs over b * Tu + to
    ("b2_brick_64_64_res", 2, 64, 64, 3, 8, 16, 3, False, False, True, True, False),
    ("b3_brick_128_64_up_thw_res", 3, 128, 64, 2, 4, 8, 3, True, True, True, True, False),
    ("b2_brick_32_32_up_hw", 2, 32, 32, 3, 4, 8, 3, False, True, False, True, True),
    ("b3_brick_64_128_up_t", 3, 64, 128, 1, 8, 16, 3, True, False, False, False, False),
    # batch > 1 row-major, M % 128 != 0, a 128-voxel tile straddles the batch boundary (105 / 240 / 90 voxels per element)
    ("b2_rows_64_64_res", 2, 64, 64, 3, 5, 7, 3, False, False, True, True, False),
    ("b3_rows_128_64_up_thw_res", 3, 128, 64, 2, 3, 5, 3, True, True, True, True, False),
    ("b3_rows_32_32_up_hw", 3, 32, 32, 2, 3, 5, 3, False, True, False, True, True),
    ("b2_rows_32_32_up_t", 2, 32, 32, 3, 5, 3, 3, True, False, False, False, False),
    ("b3_rows_k1_64_96", 3, 64, 96, 3, 5, 3, 1, False, False, False, True, True),
    # Cin = 8 / 16: 8 / 4 taps share one 64-deep K step; at Cin = 8 the K padding reaches tap indices 27 .. 31
    ("cin8_k3", 1, 8, 32, 3, 6, 7, 3, False, False, True, True, False),
    ("cin16_k3", 2, 16, 40, 2, 5, 9, 3, False, True, False, True, True),
    ("cin8_k1", 2, 8, 32, 2, 5, 7, 1, False, False, False, True, False),
    ("cin16_k1", 1, 16, 24, 3, 4, 5, 1, False, False, True, False, True),
    # Cout: the scalar epilogue away from 3, a second N tile with 2 live columns, vector-epilogue tail tiles
    ("cout6", 1, 32, 6, 2, 9, 11, 3, False, False, True, True, True),
    ("cout130", 1, 32, 130, 2, 6, 11, 3, False, False, True, True, False),
    ("cout132", 2, 32, 132, 2, 5, 5, 3, False, True, True, True, False),
    ("cout200", 1, 64, 200, 2, 8, 12, 3, False, False, False, True, True),
    # a volume thinner than the kernel
    ("thin_t1_h1", 1, 64, 64, 1, 1, 9, 3, False, False, True, True, False),
    ("thin_h1", 2, 32, 32, 3, 1, 6, 3, False, False, False, True, False),
    ("thin_w1", 1, 32, 32, 2, 7, 1, 3, False, False, False, True, True),
    ("thin_1x1x1_up_hw", 1, 64, 32, 1, 1, 1, 3, False, True, True, True, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CONV_CASES_MORE, ids=[c[0] for c in CONV_CASES_MORE])
def test_conv3d_zp_kernel_unlaunched_shapes_vs_f64(dc_ae, hip_lib, case):
    name, B, Cin, Cout, T, H, W, k, up_t, up_hw, with_res, with_bias, silu = case
    g = _gen(name)
    conv = torch.nn.Conv3d(Cin, Cout, k, bias=with_bias).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g, device=DEV) / (Cin * k ** 3) ** 0.5)
        if with_bias:
            conv.bias.copy_(0.1 * torch.randn(Cout, generator=g, device=DEV))
    plan = dc_ae._DensePlan(conv)
    x = _randn((B, T, H, W, Cin), g)
    To, Ho, Wo = T << int(up_t), H << int(up_hw), W << int(up_hw)
    brick = Ho % 8 == 0 and Wo % 16 == 0
    assert brick == ("brick" in name)
    if "rows" in name:
        assert (B * To * Ho * Wo) % 128 and (To * Ho * Wo) % 128
    res = _randn((B, To, Ho, Wo, Cout), g) if with_res else None
    guard = torch.full((B * To * Ho * Wo * Cout + 64,), float("nan"), dtype=BF, device=DEV)
    out = guard[: B * To * Ho * Wo * Cout].view(B, To, Ho, Wo, Cout)
    hip_lib.conv3d_zp(x, plan.w, plan.b, out, k, up_t, up_hw, silu, res)
    torch.cuda.synchronize()
    assert torch.isnan(guard[-64:].float()).all(), "wrote past the end of out"
    y = E.conv3d_zp_ref(x, plan.w, plan.b, k, up_t, up_hw, silu, res, dtype=torch.float64)
    _judge(name, out, y, conv_border(To, Ho, Wo, DEV) if k == 3 else None)
    if B > 1:                                                # and each element against ITS OWN single-batch formula
        for b in range(B):
            yb = E.conv3d_zp_ref(x[b: b + 1], plan.w, plan.b, k, up_t, up_hw, silu, None if res is None else res[b: b + 1],
                                 dtype=torch.float64)
            _judge(f"{name}[b={b}]", out[b: b + 1], yb, conv_border(To, Ho, Wo, DEV) if k == 3 else None)


# (name, B, C, T, H, W, ksize, glu, bias)
DW_CASES_MORE = [
    ("b2_glu_k3_256", 2, 256, 3, 5, 6, 3, True, True),
    ("b2_agg_k5_96", 2, 96, 4, 5, 6, 5, False, False),
    ("b3_plain_k3_64", 3, 64, 2, 3, 3, 3, False, True),
    ("thin_k5_w1", 1, 64, 6, 7, 1, 5, False, False),         # extents below the radius (2) of the 5-tap kernel
    ("thin_k5_t2_h1", 2, 96, 2, 1, 9, 5, False, False),
    ("thin_glu_k3_h1", 2, 64, 4, 1, 5, 3, True, True),
    ("thin_glu_k3_1x1x1", 2, 32, 1, 1, 1, 3, True, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DW_CASES_MORE, ids=[c[0] for c in DW_CASES_MORE])
def test_dwconv3d_kernel_unlaunched_shapes_vs_f64(dc_ae, hip_lib, case):
    name, B, C, T, H, W, k, glu, with_bias = case
    g = _gen(name)
    x = _randn((B, T, H, W, C), g)
    w = _randn((k ** 3, C), g, k ** -1.5)
    b = (0.1 * torch.randn(C, generator=g, device=DEV)) if with_bias else None
    out = torch.full((B, T, H, W, C // 2 if glu else C), float("nan"), dtype=BF, device=DEV)
    hip_lib.dwconv3d(x, w, b, out, k, glu)
    torch.cuda.synchronize()
    _judge(name, out, E.dwconv3d_ref(x, w, b, k, glu, dtype=torch.float64), dw_border(T, H, W, k, DEV))
    for i in range(B if B > 1 else 0):
        _judge(f"{name}[b={i}]", out[i: i + 1], E.dwconv3d_ref(x[i: i + 1], w, b, k, glu, dtype=torch.float64),
               dw_border(T, H, W, k, DEV))


def _attn_input(B, N, G, g):
    qkv = _randn((B, N, G * 96), g)
    v = qkv.view(B, N, G, 96)
    v[:, ::3, :, 32:64] = -v[:, ::3, :, 32:64].abs()        # every third token: relu(k) == 0
    v[:, :, 0, 32:64] = -v[:, :, 0, 32:64].abs()            # group 0: relu(k) == 0 for EVERY token -> 0 / (0 + eps) == 0
    return qkv


@pytest.mark.gpu
@pytest.mark.parametrize("N", [63, 64, 65, 511, 512, 513, 32769])
def test_relu_linear_attn_token_counts_at_the_tile_and_split_edges(dc_ae, hip_lib, N):
    """each side of the 64-token LDS tile and of the 512-token split, and one token past the 64-split cap (64 * 512)"""
    B, G = 2, 2
    qkv = _attn_input(B, N, G, _gen(f"la_edges{N}"))
    last = qkv.view(B, N, G, 96)[:, -1, 1, 32:64]
    last.copy_(last.abs() + 4.0)                             # the LAST token carries weight in K^T V: dropping it must show
    out = torch.full((B, N, G * 32), float("nan"), dtype=BF, device=DEV)
    hip_lib.relu_linear_attn(qkv, out)
    torch.cuda.synchronize()
    assert float(out.view(B, N, G, 32)[:, :, 0].float().abs().max()) == 0.0
    _judge(f"relu_linear_attn B{B} N{N} G{G}", out, E.relu_linear_attn_ref(qkv, dtype=torch.float64))


@pytest.mark.gpu
def test_relu_linear_attn_c_entry_point_nsplit_and_workspace(dc_ae, hip_lib):
    """osk_relu_linear_attn_bf16 itself: nsplit 1 / 7 / 64 on one input (64 runs of 64 tokens over N = 1000 leave runs 16 .. 63
    empty) agree with f64 within the bound; a workspace one byte short is refused (OSK_EINVAL = -1) and nothing is written"""
    B, N, G = 2, 1000, 3
    qkv = _attn_input(B, N, G, _gen("la_nsplit"))
    y = E.relu_linear_attn_ref(qkv, dtype=torch.float64)
    for nsplit in (1, 7, 64):
        ws = torch.full((B * G * nsplit * 1056,), float("nan"), dtype=torch.float32, device=DEV)
        out = torch.full((B, N, G * 32), float("nan"), dtype=BF, device=DEV)
        rc = hip_lib.lib.osk_relu_linear_attn_bf16(qkv.data_ptr(), B, N, G, out.data_ptr(), out.stride(1), ws.data_ptr(),
                                                   ws.numel() * 4, nsplit, 1e-15, hip_lib._stream())
        assert rc == 0, (nsplit, rc)
        torch.cuda.synchronize()
        assert torch.isfinite(ws).all(), f"nsplit {nsplit}: a partial sum was never written"
        _judge(f"relu_linear_attn nsplit {nsplit}", out, y)
        out.fill_(float("nan"))
        rc = hip_lib.lib.osk_relu_linear_attn_bf16(qkv.data_ptr(), B, N, G, out.data_ptr(), out.stride(1), ws.data_ptr(),
                                                   ws.numel() * 4 - 1, nsplit, 1e-15, hip_lib._stream())
        torch.cuda.synchronize()
        assert rc == -1 and torch.isnan(out.float()).all(), (nsplit, rc)


def _edge_rows(M, C, g, scale):
    """row 0 all zeros (only eps is left under the rsqrt); row 1 with one element 2^15 among O(1) values; the rest normal"""
    x = _randn((M, C), g, scale)
    x[0] = 0
    x[1, C // 3] = 2.0 ** 15
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("M,C,res,relu", [(5, 128, False, False), (9, 1024, True, False), (4, 32, False, True)])
def test_rmsnorm_affine_zero_row_and_outlier_row(dc_ae, hip_lib, M, C, res, relu):
    g = _gen(f"rms_edge{M}x{C}")
    x = _edge_rows(M, C, g, 1.0)
    w = 1.0 + 0.1 * torch.randn(C, generator=g, device=DEV)
    b = 0.1 * torch.randn(C, generator=g, device=DEV)
    r = _randn((M, C), g) if res else None
    out = torch.full((M, C), float("nan"), dtype=BF, device=DEV)
    hip_lib.rmsnorm_affine(x, w, b, out, 1e-5, r, relu)
    torch.cuda.synchronize()
    y = E.rmsnorm_affine_ref(x, w, b, 1e-5, r, relu, dtype=torch.float64)
    for row in range(3):                                    # each row against its own max |y|: row 1 must not set the floor
        _judge(f"rmsnorm edge rows {M}x{C} row {row}", out[row], y[row])
    _judge(f"rmsnorm edge rows {M}x{C}", out, y)


@pytest.mark.gpu
@pytest.mark.parametrize("M,C", [(3, 96), (40, 1536)])
def test_gconv32_zero_row_and_outlier_row(dc_ae, hip_lib, M, C):
    g = _gen(f"gconv_edge{M}x{C}")
    x, w = _edge_rows(M, C, g, 1.0), _randn((C, 32), g, 32 ** -0.5)
    out = torch.full((M, C), float("nan"), dtype=BF, device=DEV)
    hip_lib.gconv32(x, w, out)
    torch.cuda.synchronize()
    y = E.gconv32_ref(x, w, dtype=torch.float64)
    assert float(out[0].float().abs().max()) == 0.0
    grp = (C // 3) // 32
    for row in range(3):
        _judge(f"gconv32 edge rows {M}x{C} row {row}", out[row], y[row])
    others = torch.ones(C, dtype=torch.bool, device=DEV)
    others[grp * 32: grp * 32 + 32] = False                  # row 1 outside the outlier's group: O(1) values, their own floor
    _judge(f"gconv32 edge rows {M}x{C} row 1, other groups", out[1][others], y[1][others])
    _judge(f"gconv32 edge rows {M}x{C}", out, y)


# ------------------------------------------------------------------------------------------------------------ the decoder
def _small_model(dc_ae, **kw):
    c = R.SMALL
    dec = dc_ae.DecoderConfig(in_channels=3, latent_channels=c["latent_channels"], width_list=c["width_list"],
                              depth_list=c["depth_list"], block_type=list(c["block_type"]), norm="rms3d", act="silu",
                              upsample_block_type="InterpolateConv", out_norm="rms3d", is_video=True,
                              temporal_upsample=c["temporal_upsample"])
    cfg = dc_ae.DCAEConfig(in_channels=3, latent_channels=c["latent_channels"], time_compression_ratio=4,
                           spatial_compression_ratio=32, decoder=dec, **kw)
    with torch.device(DEV):
        m = dc_ae.DCAE(cfg).to(BF)
    m.load_state_dict(R.make_state_dict(R.param_shapes(R.SMALL)))
    return m


def _restated(cfg, z, dtype, tiled=False, seed=0):
    sd = {k: v.to(dtype) for k, v in R.make_state_dict(R.param_shapes(cfg), seed).items()}
    fn = lambda t: R.decode(sd, cfg, t)  # noqa: E731
    with torch.no_grad():
        if not tiled:
            return fn(z.to(dtype))
        return R.tiled_decode(fn, z.to(dtype), spatial=True, temporal=True, spatial_tile_size=128, temporal_tile_size=16,
                              spatial_tile_latent_size=4, temporal_tile_latent_size=4)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["a", "b"], ids=["untiled", "single_frame"])
def test_decode_small_geometry_against_reference_golden(dc_ae, tag):
    g = np.load(GOLDEN)
    z = torch.from_numpy(g["z_" + tag])
    with torch.inference_mode():
        ours = _small_model(dc_ae).decode(z.to(DEV, BF))
    torch.cuda.synchronize()
    want = torch.from_numpy(g["dec_" + tag])
    assert ours.dtype == BF and tuple(ours.shape) == tuple(want.shape)
    assert_parity(ours, want, finite_retry(lambda: _restated(R.SMALL, z, BF)), f"dc_ae small decode ({tag})")


@pytest.mark.gpu
def test_tiled_decode_small_geometry_against_reference_golden(dc_ae):
    g = np.load(GOLDEN)
    z = torch.from_numpy(g["z_c"])
    with torch.inference_mode():
        ours = _small_model(dc_ae, use_spatial_tiling=True, use_temporal_tiling=True, **TILED).decode(z.to(DEV, BF))
    torch.cuda.synchronize()
    assert tuple(ours.shape) == (1, 3, 24, 192, 160)
    ref = finite_retry(lambda: _restated(R.SMALL, z, BF, tiled=True))
    ti, ri, ci = (torch.as_tensor(g[k]) for k in ("tiled_t", "tiled_rows", "tiled_cols"))

    def subset(d):
        d = d.cpu()[:, :, ti]
        return d[:, :, :, ri, :], d[:, :, :, :, ci]

    for o, r, key in zip(subset(ours), subset(ref), ("dec_c_rows", "dec_c_cols")):
        assert_parity(o, torch.from_numpy(g[key]), r, f"dc_ae small tiled decode ({key})")


@pytest.mark.gpu
def test_decode_shipped_widths_reduced_latent(dc_ae):
    """dc-ae-f32t4c128 as the factory builds it, latent [1, 128, 2, 4, 4] -> [1, 3, 8, 128, 128], against the fp32 restatement"""
    m = dc_ae.DC_AE("dc-ae-f32t4c128", device_map=DEV, torch_dtype=BF, from_scratch=True)
    m.load_state_dict(R.make_state_dict(R.param_shapes(R.SHIPPED), seed=1))
    z = torch.randn(1, 128, 2, 4, 4, generator=torch.Generator().manual_seed(5)).bfloat16().float()
    with torch.inference_mode():
        ours = m.decode(z.to(DEV, BF))
    torch.cuda.synchronize()
    assert ours.dtype == BF and tuple(ours.shape) == (1, 3, 8, 128, 128)
    truth = _restated(R.SHIPPED, z, torch.float32, seed=1)
    ref = finite_retry(lambda: _restated(R.SHIPPED, z, BF, seed=1))
    assert_parity(ours, truth, ref, "dc_ae shipped widths, latent 2 x 4 x 4")
