"""CPU: host side of the Video DC-AE decoder (open_sora_amd.dc_ae), driven through the CPU emulation of the kernels' semantics
(tests/cpu_ops_dc_ae.py), and the plain-torch restatement the GPU tests take as truth (tests/dc_ae_restatement.py) pinned to the
reference's committed output (tests/golden/dc_ae_small.npz, recorded by tools/make_golden_dc_ae.py) and, where the reference tree
is present, to the live reference.  The kernels themselves are checked on the GPU by tests/test_gpu_dc_ae.py."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_loader
from tests import cpu_ops_dc_ae
from tests import dc_ae_restatement as R
from tests.util import assert_parity, finite_retry, rel_l2

BF = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dc_ae_small.npz")
needs_ref = pytest.mark.skipif(not ref_loader.available(), reason="needs the reference tree (oracle.ref_loader)")
TILED = dict(spatial_tile_size=128, temporal_tile_size=16, tile_overlap_factor=0.25)


@pytest.fixture()
def emu(hip_lib):
    from open_sora_amd import dc_ae, mmdit

    mmdit.set_ops_for_testing(cpu_ops_dc_ae)
    yield dc_ae
    mmdit.set_ops_for_testing(hip_lib)


@pytest.fixture(scope="module")
def golden():
    return {k: v for k, v in np.load(GOLDEN).items()}


def small_cfg(D, **kw):
    c = R.SMALL
    dec = D.DecoderConfig(in_channels=3, latent_channels=c["latent_channels"], width_list=c["width_list"], depth_list=c["depth_list"],
                          block_type=list(c["block_type"]), norm="rms3d", act="silu", upsample_block_type="InterpolateConv",
                          out_norm="rms3d", is_video=True, temporal_upsample=c["temporal_upsample"])
    return D.DCAEConfig(in_channels=3, latent_channels=c["latent_channels"], time_compression_ratio=4, spatial_compression_ratio=32,
                        decoder=dec, **kw)


def small_model(D, dtype=torch.float32, **kw):
    m = D.DCAE(small_cfg(D, **kw)).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in R.make_state_dict(R.param_shapes(R.SMALL)).items()})
    return m


def restated(z, dtype=torch.float32, tiled=False):
    sd = {k: v.to(dtype) for k, v in R.make_state_dict(R.param_shapes(R.SMALL)).items()}
    fn = lambda t: R.decode(sd, R.SMALL, t)  # noqa: E731
    with torch.no_grad():
        if not tiled:
            return fn(z.to(dtype))
        return R.tiled_decode(fn, z.to(dtype), spatial=True, temporal=True, spatial_tile_size=128, temporal_tile_size=16,
                              spatial_tile_latent_size=4, temporal_tile_latent_size=4)


def tiled_subset(dec, g):
    d = dec[:, :, torch.as_tensor(g["tiled_t"])]
    return d[:, :, :, torch.as_tensor(g["tiled_rows"]), :], d[:, :, :, :, torch.as_tensor(g["tiled_cols"])]


# ------------------------------------------------------------------------------------------------- restatement == reference
def test_restatement_matches_reference_golden(golden):
    for tag in ("a", "b"):
        out = restated(torch.from_numpy(golden["z_" + tag]))
        want = torch.from_numpy(golden["dec_" + tag])
        assert out.shape == want.shape
        assert rel_l2(out, want) <= 1e-5, (tag, rel_l2(out, want))
    out = restated(torch.from_numpy(golden["z_c"]), tiled=True)
    assert tuple(out.shape) == (1, 3, 24, 192, 160)
    by_rows, by_cols = tiled_subset(out, golden)
    assert rel_l2(by_rows, torch.from_numpy(golden["dec_c_rows"])) <= 1e-5
    assert rel_l2(by_cols, torch.from_numpy(golden["dec_c_cols"])) <= 1e-5


def test_restatement_tap_sum_convs_match_reference_golden(golden):
    """decode(taps=True), the form the operating-point GPU tests evaluate: in fp32 the same output as through F.conv3d; in
    bf16 a comparator of the same precision (its error against the golden is not larger than F.conv3d's by more than 25 %)"""
    sd = R.make_state_dict(R.param_shapes(R.SMALL))
    sd_b = {k: v.to(BF) for k, v in sd.items()}
    with torch.no_grad():
        for tag in ("a", "b"):
            z, want = torch.from_numpy(golden["z_" + tag]), torch.from_numpy(golden["dec_" + tag])
            out = R.decode(sd, R.SMALL, z, taps=True)
            assert rel_l2(out, want) <= 1e-5
            assert rel_l2(out, R.decode(sd, R.SMALL, z)) <= 1e-5
            e_taps = rel_l2(R.decode(sd_b, R.SMALL, z.to(BF), taps=True), want)
            e_conv = rel_l2(finite_retry(lambda: R.decode(sd_b, R.SMALL, z.to(BF))), want)
            print(f"bf16 restatement ({tag}): relL2 taps {e_taps:.3e} F.conv3d {e_conv:.3e}")
            assert e_taps <= 1.25 * e_conv
        g = torch.Generator().manual_seed(4)
        x, w, b = torch.randn(2, 64, 3, 4, 5, generator=g), torch.randn(6, 64, 3, 3, 3, generator=g), torch.randn(6, generator=g)
        assert rel_l2(R.conv_same_taps(x, w, b), R.conv_same(x, w, b)) <= 1e-6                                  # dense
        assert rel_l2(R.conv_same_taps(x, w[:, :, :1, :1, :1]), R.conv_same(x, w[:, :, :1, :1, :1])) <= 1e-6     # 1x1x1
        wd = torch.randn(64, 1, 5, 5, 5, generator=g)
        assert rel_l2(R.conv_same_taps(x, wd, None, 64), R.conv_same(x, wd, None, 64)) <= 1e-6                   # depthwise
        wg = torch.randn(64, 32, 1, 1, 1, generator=g)
        assert rel_l2(R.conv_same_taps(x, wg, None, 2), R.conv_same(x, wg, None, 2)) <= 1e-6                     # grouped


@needs_ref
def test_restatement_matches_live_reference():
    from tools.make_golden_dc_ae import reference_dcae

    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        ref, _ = reference_dcae(R.SMALL)
        for shape in ((1, 32, 3, 2, 3), (1, 32, 1, 3, 2)):
            z = torch.randn(shape, generator=g)
            assert rel_l2(restated(z), ref.decode(z)) <= 1e-5
        tiled, _ = reference_dcae(R.SMALL, use_spatial_tiling=True, use_temporal_tiling=True, **TILED)
        z = torch.randn(1, 32, 5, 5, 6, generator=g)
        assert rel_l2(restated(z, tiled=True), tiled.decode(z)) <= 1e-5


# ------------------------------------------------------------------------------------------------------------- state dict
def test_state_dict_keys_match_recorded_reference_keys(emu, golden):
    want = [str(k) for k in golden["keys"]]
    ours = small_model(emu).state_dict()
    assert list(ours) == want
    shapes = R.param_shapes(R.SMALL)
    assert list(shapes) == want
    assert {k: tuple(v.shape) for k, v in ours.items()} == {k: tuple(v) for k, v in shapes.items()}


def test_shipped_config_keys_and_issue_examples(emu):
    with torch.device("meta"):
        m = emu.DCAE(emu.dc_ae_f32("dc-ae-f32t4c128", None))
    sd = m.state_dict()
    shapes = R.param_shapes(R.SHIPPED)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v) for k, v in shapes.items()}
    for k in ("decoder.project_in.main.conv.weight", "decoder.stages.3.op_list.1.context_module.main.aggreg.0.1.weight",
              "decoder.stages.4.op_list.2.local_module.main.point_conv.norm.bias", "decoder.project_out.op_list.2.conv.bias"):
        assert k in sd, k
    assert tuple(sd["decoder.stages.3.op_list.1.context_module.main.aggreg.0.1.weight"].shape) == (1536, 32, 1, 1, 1)


@needs_ref
def test_shipped_config_keys_match_live_reference(emu):
    from tools.make_golden_dc_ae import reference_module

    D = reference_module()
    with torch.device("meta"):
        ref = D.Decoder(D.DecoderConfig(**{k: (list(v) if k == "block_type" else v) for k, v in R.SHIPPED.items()}, norm="rms3d",
                                        act="silu", upsample_block_type="InterpolateConv", out_norm="rms3d", is_video=True))
        ours = emu.DCAE(emu.dc_ae_f32("dc-ae-f32t4c128", None))
    a = {"decoder." + k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert a == {k: tuple(v.shape) for k, v in ours.state_dict().items()}


def test_dc_ae_f32_field_values(emu):
    c = emu.dc_ae_f32("dc-ae-f32t4c128", "some/path.pt")
    assert (c.time_compression_ratio, c.spatial_compression_ratio, c.latent_channels, c.in_channels) == (4, 32, 128, 3)
    assert c.pretrained_path == "some/path.pt" and c.scaling_factor is None and not c.use_quant_conv
    d = c.decoder
    assert tuple(d.width_list) == (128, 256, 512, 512, 1024, 1024) and tuple(d.depth_list) == (3, 3, 3, 3, 3, 3)
    assert list(d.block_type) == ["ResBlock"] * 3 + ["EViTS5_GLU"] * 3
    assert (d.upsample_block_type, d.norm, d.act, d.out_norm, d.out_act, d.is_video) == ("InterpolateConv", "rms3d", "silu", "rms3d",
                                                                                        "relu", True)
    assert tuple(d.temporal_upsample) == (False, False, False, True, True, False) and d.latent_channels == 128
    assert (d.in_shortcut, d.upsample_shortcut, d.upsample_match_channel) == ("duplicating", "duplicating", True)
    e = c.encoder
    assert tuple(e.depth_list) == (2, 2, 2, 3, 3, 3) and e.downsample_block_type == "Conv" and e.norm == "rms3d" and e.is_video
    assert (c.spatial_tile_size, c.temporal_tile_size, c.tile_overlap_factor) == (256, 32, 0.25)
    with pytest.raises(NotImplementedError):
        emu.dc_ae_f32("dc-ae-f64c128", None)


def test_factory_mirrors_reference_arguments(emu):
    import inspect

    names = list(inspect.signature(emu.DC_AE).parameters)
    assert names == ["model_name", "device_map", "torch_dtype", "from_scratch", "from_pretrained", "is_training", "use_spatial_tiling",
                     "use_temporal_tiling", "spatial_tile_size", "temporal_tile_size", "tile_overlap_factor", "scaling_factor",
                     "disc_off_grad_ckpt"]
    m = emu.DC_AE("dc-ae-f32t4c128", device_map="meta", from_scratch=True, use_spatial_tiling=True, use_temporal_tiling=True,
                  spatial_tile_size=128, scaling_factor=0.5)
    assert m.use_spatial_tiling and m.use_temporal_tiling and m.spatial_tile_size == 128 and m.scaling_factor == 0.5
    # as in the reference, the latent tile sizes were derived from the CONFIG at construction
    assert (m.spatial_tile_latent_size, m.temporal_tile_latent_size) == (8, 8)
    assert m.get_latent_size([128, 768, 768]) == [32, 24, 24] and m.get_latent_size([1, 256, 250]) == [1, 8, 8]
    with pytest.raises(ValueError, match="from_pretrained"):
        emu.DC_AE("dc-ae-f32t4c128", device_map="meta")


# ----------------------------------------------------------------------------------------------------- loading / refusals
def test_encode_raises_and_encoder_keys_are_dropped(emu):
    m = small_model(emu)
    with pytest.raises(NotImplementedError, match="DECODER"):
        m.encode(torch.zeros(1, 3, 4, 32, 32))
    sd = R.make_state_dict(R.param_shapes(R.SMALL), seed=5)
    full = dict(sd)
    full["encoder.project_in.conv.weight"] = torch.zeros(32, 3, 3, 3, 3)
    full["encoder.stages.0.op_list.0.main.conv1.conv.bias"] = torch.zeros(32)
    m.load_state_dict(full)                                   # strict: passes because encoder.* is dropped
    got = m.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in sd) and not any(k.startswith("encoder.") for k in got)
    bad = dict(sd)
    bad["quant_conv.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match="quant_conv"):
        m.load_state_dict(bad)
    short = dict(sd)
    short.pop("decoder.project_in.main.conv.bias")
    with pytest.raises(RuntimeError, match="project_in"):
        m.load_state_dict(short)


def test_checkpoint_file_with_encoder_keys_loads(emu, tmp_path):
    from safetensors.torch import save_file

    from open_sora_amd.ckpt import load_checkpoint

    sd = R.make_state_dict(R.param_shapes(R.SMALL), seed=2)
    full = {k: v.contiguous() for k, v in sd.items()}
    full["encoder.project_in.conv.weight"] = torch.zeros(32, 3, 3, 3, 3)
    path = str(tmp_path / "dcae.safetensors")
    save_file(full, path)
    m = load_checkpoint(emu.DCAE(small_cfg(emu)), path, device_map="cpu")
    got = m.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


@pytest.mark.parametrize("field,value,match", [
    ("width_list", (32, 32, 64, 64, 64, 96), "width 96"),
    ("block_type", ["ResBlock"] * 5 + ["EViT_GLU"], "block_type 'EViT_GLU'"),
    ("norm", "bn2d", "norm 'bn2d'"),
    ("act", "relu6", "activation 'relu6'"),
    ("upsample_block_type", "ConvPixelShuffle", "upsample_block_type"),
    ("is_video", False, "2-D image decoder"),
    ("out_norm", "rms2d", "project_out"),
    ("latent_channels", 24, "latent_channels 24"),
])
def test_unsupported_configurations_are_refused_at_construction(emu, field, value, match):
    cfg = small_cfg(emu)
    setattr(cfg.decoder, field, value)
    with pytest.raises(ValueError, match=match):
        emu.DCAE(cfg)


# --------------------------------------------------------------------------------------------------------------- tile loop
def _stub(z):
    """a deterministic `_decode`: the first three latent channels, nearest-upsampled 4 x 32 x 32 (bf16-representable)"""
    return z[:, :3].repeat_interleave(4, 2).repeat_interleave(32, 3).repeat_interleave(32, 4).contiguous()


TILE_CASES = [
    # latent shape, spatial, temporal tiling, pixel tile sizes, latent tile sizes (config-derived)
    ((1, 4, 6, 6, 5), True, True, 128, 16),       # short last tile on every axis
    ((1, 4, 7, 4, 9), True, True, 128, 16),       # last temporal tile of ONE latent frame; H fits in one tile
    ((1, 4, 3, 10, 10), True, False, 128, 16),    # spatial only, 4 x 4 tiles, the last of one latent row / column
    ((1, 4, 13, 3, 3), False, True, 128, 16),     # temporal only
    ((1, 4, 9, 9, 9), True, True, 256, 32),       # the shipped tile sizes: one latent row / column / frame spills over
    ((1, 4, 4, 4, 4), True, True, 128, 16),       # nothing exceeds a tile: no tiling
]


@pytest.mark.parametrize("shape,sp,tp,sts,tts", TILE_CASES)
def test_tile_loop_matches_restatement(emu, monkeypatch, shape, sp, tp, sts, tts):
    m = small_model(emu, use_spatial_tiling=sp, use_temporal_tiling=tp, spatial_tile_size=sts, temporal_tile_size=tts)
    calls = []

    def stub(z):
        calls.append(tuple(z.shape))
        return _stub(z)

    monkeypatch.setattr(m, "_decode", stub)
    z = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(BF)
    out = m.decode(z.clone())
    want_calls = []

    def stub32(t):
        want_calls.append(tuple(t.shape))
        return _stub(t)

    want = R.tiled_decode(stub32, z.float(), spatial=sp, temporal=tp, spatial_tile_size=sts, temporal_tile_size=tts,
                          spatial_tile_latent_size=sts // 32, temporal_tile_latent_size=tts // 4)
    assert calls == want_calls                     # the same tiles, in the same order, short last tiles included
    assert out.dtype == BF and out.shape == want.shape
    # the cross-fades run in f32 with one bf16 rounding per fade (two where a vertical and a horizontal fade overlap)
    assert rel_l2(out, want) <= 2 * 2.0 ** -9, rel_l2(out, want)
    assert float((out.float() - want).abs().max()) <= 2 * 2.0 ** -8 * float(want.abs().max())


@needs_ref
@pytest.mark.parametrize("shape,sp,tp,sts,tts", TILE_CASES)
def test_tile_loop_matches_live_reference(emu, monkeypatch, shape, sp, tp, sts, tts):
    from tools.make_golden_dc_ae import reference_dcae

    ref, _ = reference_dcae(R.SMALL, use_spatial_tiling=sp, use_temporal_tiling=tp, spatial_tile_size=sts, temporal_tile_size=tts)
    m = small_model(emu, use_spatial_tiling=sp, use_temporal_tiling=tp, spatial_tile_size=sts, temporal_tile_size=tts)
    for k in ("spatial_tile_latent_size", "temporal_tile_latent_size", "spatial_tile_size", "temporal_tile_size", "tile_overlap_factor"):
        assert getattr(m, k) == getattr(ref, k), k
    ours_calls, ref_calls = [], []
    monkeypatch.setattr(m, "_decode", lambda t: (ours_calls.append(tuple(t.shape)), _stub(t))[1])
    monkeypatch.setattr(ref, "_decode", lambda t: (ref_calls.append(tuple(t.shape)), _stub(t))[1])
    z = torch.randn(shape, generator=torch.Generator().manual_seed(2)).to(BF)
    out, want = m.decode(z.clone()), ref.decode(z.float())
    assert ours_calls == ref_calls and out.shape == want.shape
    assert rel_l2(out, want) <= 2 * 2.0 ** -9


# ------------------------------------------------------------------------------- the decoder through the emulated kernels
@pytest.mark.parametrize("tag", ["a", "b"])
def test_emulated_decode_matches_golden(emu, golden, tag):
    z = torch.from_numpy(golden["z_" + tag])
    with torch.no_grad():
        out = small_model(emu, BF).decode(z.to(BF))
    assert out.dtype == BF
    ref_bf16 = finite_retry(lambda: restated(z, BF))
    assert_parity(out, torch.from_numpy(golden["dec_" + tag]), ref_bf16, f"emulated decode {tag}")


def test_emulated_tiled_decode_matches_golden(emu, golden):
    z = torch.from_numpy(golden["z_c"])
    with torch.no_grad():
        m = small_model(emu, BF, use_spatial_tiling=True, use_temporal_tiling=True, **TILED)
        out = m.decode(z.to(BF))
    assert tuple(out.shape) == (1, 3, 24, 192, 160)
    ref_bf16 = finite_retry(lambda: restated(z, BF, tiled=True))
    for ours, ref, key in zip(tiled_subset(out, golden), tiled_subset(ref_bf16, golden), ("dec_c_rows", "dec_c_cols")):
        assert_parity(ours, torch.from_numpy(golden[key]), ref, f"emulated tiled decode {key}")
