"""GPU: the Video DC-AE encoder (open_sora_amd.dc_ae with build_encoder=True, csrc/dc_ae.hip) on the MI355X.

- the two new kernels against an f64 evaluation of the formula of include/osk.h on bf16-representable inputs, under the bound
  of tests/dc_ae_audit._judge (|out - y| <= 2^-8 |y| + 1e-4 max|y|); the conv cases judge the border voxels separately;
- the small-geometry encode (untiled, single frame, T = 2, tiled) against the committed fixture the reference itself produced;
- the shipped-width encode on a reduced input against the plain-torch fp32 restatement (tests/dc_ae_enc_restatement.py);
  tolerance: tests.util.assert_parity with the restatement in bf16 (CPU, never the code under test) as the comparator.
No test here reads the reference tree."""
import os
import zlib

import numpy as np
import pytest
import torch

from tests import cpu_ops_dc_ae_enc as E
from tests import dc_ae_enc_restatement as RE
from tests import dc_ae_restatement as R
from tests.dc_ae_audit import _judge, conv_border
from tests.util import assert_parity, finite_retry
from tools.make_golden_dc_ae_enc import SUB, input_d, small_state_dict

BF = torch.bfloat16
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dc_ae_enc_small.npz")
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


# (name, Cin, Cout, B, T, H, W (source), stride_t, res, bias)
STRIDED_CASES = [
    ("down_128_256_brick", 128, 256, 1, 3, 16, 32, 1, True, True),        # 8 x 16 outputs per frame: brick path, three tiles
    ("down_512_1024_t", 512, 1024, 1, 4, 8, 8, 2, True, True),            # 32 rows, one partial tile
    ("down_512_1024_t_single_frame", 512, 1024, 1, 1, 4, 6, 2, True, True),  # temporal stride on one frame: taps pad, frame, pad
    ("down_64_64_t2_to_1", 64, 64, 1, 2, 4, 4, 2, True, True),
    ("down_32_32_odd", 32, 32, 1, 5, 7, 9, 2, True, True),                # the small-Cin path; odd extents: the far padding is read
    ("down_256_512_odd_nores", 256, 512, 1, 2, 5, 7, 1, False, True),
    ("down_32_192_129_rows", 32, 192, 1, 1, 6, 86, 1, True, True),        # 129 output voxels; a Cout tail past 128
    ("down_64_128_b2", 64, 128, 2, 2, 4, 4, 2, True, True),               # the batch boundary under the temporal pad
    ("down_128_128_nobias", 128, 128, 1, 2, 6, 10, 2, True, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", STRIDED_CASES, ids=[c[0] for c in STRIDED_CASES])
def test_conv3d_zp_strided_kernel_vs_f64(dc_ae, hip_lib, case):
    name, Cin, Cout, B, T, H, W, st, with_res, with_bias = case
    g = _gen(name)
    conv = torch.nn.Conv3d(Cin, Cout, 3, bias=with_bias).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g, device=DEV) / (Cin * 27) ** 0.5)
        if with_bias:
            conv.bias.copy_(0.1 * torch.randn(Cout, generator=g, device=DEV))
    plan = dc_ae._DensePlan(conv)
    x = _randn((B, T, H, W, Cin), g)
    To, Ho, Wo = (T - 1) // st + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert (Ho % 8 == 0 and Wo % 16 == 0) == ("brick" in name)
    res = _randn((B, To, Ho, Wo, Cout), g) if with_res else None
    n = B * To * Ho * Wo * Cout
    guard = torch.full((n + 64,), float("nan"), dtype=BF, device=DEV)
    out = guard[:n].view(B, To, Ho, Wo, Cout)
    hip_lib.conv3d_zp_strided(x, plan.w, plan.b, out, st, res)
    torch.cuda.synchronize()
    assert torch.isnan(guard[-64:].float()).all(), "wrote past the end of out"
    y = E.conv3d_zp_strided_ref(x, plan.w, plan.b, st, 2, res, dtype=torch.float64)
    assert y.shape == out.shape
    _judge(name, out, y, conv_border(To, Ho, Wo, DEV))
    for b in range(B if B > 1 else 0):                       # and each element against ITS OWN single-batch formula
        yb = E.conv3d_zp_strided_ref(x[b: b + 1], plan.w, plan.b, st, 2, None if res is None else res[b: b + 1], dtype=torch.float64)
        _judge(f"{name}[b={b}]", out[b: b + 1], yb, conv_border(To, Ho, Wo, DEV))


# (name, Cin, Cout, B, T, H, W, ft, fhw)
AVG_CASES = [
    ("down_128_256_2d", 128, 256, 1, 3, 6, 10, 1, 2),
    ("down_512_1024_3d_gs4", 512, 1024, 1, 4, 4, 6, 2, 2),
    ("down_1024_1024_2d_t1", 1024, 1024, 1, 1, 6, 4, 1, 2),
    ("project_out_1024_128_gs8", 1024, 128, 1, 3, 5, 3, 1, 1),
    ("down_32_32_2d_gs4", 32, 32, 1, 2, 10, 14, 1, 2),
    ("down_64_128_2d_b2_odd_t", 64, 128, 2, 3, 4, 6, 1, 2),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", AVG_CASES, ids=[c[0] for c in AVG_CASES])
def test_unshuffle_avg_kernel_vs_f64_and_restatement(dc_ae, hip_lib, case):
    name, Cin, Cout, B, T, H, W, ft, fhw = case
    x = _randn((B, T, H, W, Cin), _gen(name))
    out = torch.full((B, T // ft, H // fhw, W // fhw, Cout), float("nan"), dtype=BF, device=DEV)
    hip_lib.unshuffle_avg(x, out, ft, fhw)
    torch.cuda.synchronize()
    _judge(name + " vs index formula", out, E.unshuffle_avg_ref(x, Cout, ft, fhw, dtype=torch.float64))
    want = RE.avg_shortcut(x.permute(0, 4, 1, 2, 3).double(), Cout, fhw, ft == 2).permute(0, 2, 3, 4, 1)
    _judge(name + " vs restatement", out, want)


@pytest.mark.gpu
def test_encoder_kernels_refuse_without_launch(dc_ae, hip_lib):
    lib, s = hip_lib.lib, hip_lib._stream()
    EINVAL = -1                                               # OSK_EINVAL of csrc/osk_common.h
    x = torch.randn(1, 2, 4, 4, 24, device=DEV).to(BF)
    w = torch.zeros(8, 27 * 32, dtype=BF, device=DEV)
    out = torch.zeros(4096, dtype=BF, device=DEV)

    def conv(Cin, st, shw):
        return lib.osk_conv3d_zp_strided_ndhwc_bf16(x.data_ptr(), 1, 2, 4, 4, Cin, w.data_ptr(), w.stride(0), None, 8, st, shw, None,
                                                    out.data_ptr(), s)

    def avg(T, Cin, Cout, ft, fhw):
        return lib.osk_unshuffle_avg_ndhwc_bf16(x.data_ptr(), 1, T, 2, 2, Cin, out.data_ptr(), Cout, ft, fhw, s)

    assert conv(24, 2, 2) == hip_lib.OSK_EUNSUPPORTED          # Cin = 24 is not 8 * 2^j
    assert conv(16, 2, 1) == EINVAL                # stride_hw = 1
    assert conv(16, 3, 2) == EINVAL                # stride_t = 3
    assert avg(2, 24, 64, 1, 2) == EINVAL          # gs = 24 * 4 / 64 is not whole
    assert avg(2, 24, 12, 1, 2) == hip_lib.OSK_EUNSUPPORTED    # Cout % 8
    assert avg(3, 16, 16, 2, 2) == EINVAL          # odd T with ft = 2
    torch.cuda.synchronize()
    assert float(out.float().abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------------------ the encoder
def _small_model(dc_ae, **kw):
    e, d = RE.SMALL, R.SMALL
    enc = dc_ae.EncoderConfig(in_channels=3, latent_channels=e["latent_channels"], width_list=e["width_list"],
                              depth_list=e["depth_list"], block_type=list(e["block_type"]), norm="rms3d", act="silu",
                              downsample_block_type="Conv", is_video=True, temporal_downsample=e["temporal_downsample"])
    dec = dc_ae.DecoderConfig(in_channels=3, latent_channels=d["latent_channels"], width_list=d["width_list"],
                              depth_list=d["depth_list"], block_type=list(d["block_type"]), norm="rms3d", act="silu",
                              upsample_block_type="InterpolateConv", out_norm="rms3d", is_video=True,
                              temporal_upsample=d["temporal_upsample"])
    cfg = dc_ae.DCAEConfig(in_channels=3, latent_channels=e["latent_channels"], time_compression_ratio=4,
                           spatial_compression_ratio=32, encoder=enc, decoder=dec, build_encoder=True, **kw)
    with torch.device(DEV):
        m = dc_ae.DCAE(cfg).to(BF)
    m.load_state_dict(small_state_dict())
    return m


def _restated(cfg, x, dtype, tiled=False, seed=0):
    sd = {k: v.to(dtype) for k, v in R.make_state_dict(RE.enc_param_shapes(cfg), seed).items()}
    fn = lambda t: RE.encode(sd, cfg, t)  # noqa: E731
    with torch.no_grad():
        if not tiled:
            return fn(x.to(dtype))
        return RE.tiled_encode(fn, x.to(dtype), spatial=True, temporal=True, spatial_tile_size=128, temporal_tile_size=16,
                               spatial_tile_latent_size=4, temporal_tile_latent_size=4)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["a", "b", "c"], ids=["untiled", "single_frame", "two_frames"])
def test_encode_small_geometry_against_reference_golden(dc_ae, tag):
    g = np.load(GOLDEN)
    x = torch.from_numpy(g["x_" + tag])
    with torch.inference_mode():
        ours = _small_model(dc_ae).encode(x.to(DEV, BF))
    torch.cuda.synchronize()
    want = torch.from_numpy(g["z_" + tag])
    assert ours.dtype == BF and tuple(ours.shape) == tuple(want.shape)
    assert_parity(ours, want, finite_retry(lambda: _restated(RE.SMALL, x, BF)), f"dc_ae small encode ({tag})")


@pytest.mark.gpu
def test_tiled_encode_small_geometry_against_reference_golden(dc_ae):
    g = np.load(GOLDEN)
    x = input_d()
    assert np.array_equal(x.flatten()[::SUB].numpy(), g["x_d_sub"]), "the seeded generator no longer reproduces the input of d"
    with torch.inference_mode():
        ours = _small_model(dc_ae, use_spatial_tiling=True, use_temporal_tiling=True, **TILED).encode(x.to(DEV, BF))
    torch.cuda.synchronize()
    assert ours.dtype == BF and tuple(ours.shape) == (1, 32, 5, 5, 4)
    ref = finite_retry(lambda: _restated(RE.SMALL, x, BF, tiled=True))
    assert_parity(ours, torch.from_numpy(g["z_d"]), ref, "dc_ae small tiled encode (d)")


@pytest.mark.gpu
def test_encode_shipped_widths_reduced_input(dc_ae):
    """dc-ae-f32t4c128 as the factory builds it, [1, 3, 4, 64, 64] -> [1, 128, 1, 2, 2], against the fp32 restatement; and
    scaling_factor divides the latent (one more bf16 rounding)"""
    m = dc_ae.DC_AE_with_encoder("dc-ae-f32t4c128", device_map=DEV, torch_dtype=BF, from_scratch=True)
    sd = dict(R.make_state_dict(RE.enc_param_shapes(RE.SHIPPED), seed=1))
    sd.update(R.make_state_dict(R.param_shapes(R.SHIPPED), seed=1))
    m.load_state_dict(sd)
    x = torch.randn(1, 3, 4, 64, 64, generator=torch.Generator().manual_seed(5)).bfloat16().float()
    with torch.inference_mode():
        ours = m.encode(x.to(DEV, BF))
        m.scaling_factor = 0.41407
        scaled = m.encode(x.to(DEV, BF))
    torch.cuda.synchronize()
    assert ours.dtype == BF and tuple(ours.shape) == (1, 128, 1, 2, 2)
    truth = _restated(RE.SHIPPED, x, torch.float32, seed=1)
    ref = finite_retry(lambda: _restated(RE.SHIPPED, x, BF, seed=1))
    assert_parity(ours, truth, ref, "dc_ae shipped widths, input 4 x 64 x 64")
    assert torch.equal(scaled, ours / 0.41407)                # the same division on the same bf16 latent: one rounding


@pytest.mark.gpu
def test_forward_round_trip_small_geometry(dc_ae):
    x = torch.randn(1, 3, 8, 32, 32, generator=torch.Generator().manual_seed(9)).to(DEV)
    m = _small_model(dc_ae)
    with torch.inference_mode():
        dec, mid, z = m(x)
        again = m.encode(x.to(BF))
    torch.cuda.synchronize()
    assert mid is None and dec.shape == x.shape and dec.dtype == x.dtype
    assert tuple(z.shape) == (1, 32, 2, 1, 1) and torch.equal(z, again)
