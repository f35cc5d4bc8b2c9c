"""CPU: host side of the Video DC-AE encoder (open_sora_amd.dc_ae with build_encoder=True), driven through the CPU emulation of
the kernels' semantics (tests/cpu_ops_dc_ae_enc.py), and the plain-torch restatement the GPU tests take as truth
(tests/dc_ae_enc_restatement.py) pinned to the reference's committed output (tests/golden/dc_ae_enc_small.npz, recorded by
tools/make_golden_dc_ae_enc.py) and, where the reference tree is present, to the live reference.  The kernels themselves are
checked on the GPU by tests/test_gpu_dc_ae_encoder.py."""
import inspect
import os

import numpy as np
import pytest
import torch

from oracle import ref_loader
from tests import cpu_ops_dc_ae_enc
from tests import dc_ae_enc_restatement as RE
from tests import dc_ae_restatement as R
from tests.util import assert_parity, finite_retry, rel_l2
from tools.make_golden_dc_ae_enc import SHAPES, SUB, input_d, small_state_dict

BF = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dc_ae_enc_small.npz")
needs_ref = pytest.mark.skipif(not ref_loader.available(), reason="needs the reference tree (oracle.ref_loader)")
TILED = dict(spatial_tile_size=128, temporal_tile_size=16, tile_overlap_factor=0.25)


@pytest.fixture()
def emu(hip_lib):
    from open_sora_amd import dc_ae, mmdit

    mmdit.set_ops_for_testing(cpu_ops_dc_ae_enc)
    yield dc_ae
    mmdit.set_ops_for_testing(hip_lib)


@pytest.fixture(scope="module")
def golden():
    return {k: v for k, v in np.load(GOLDEN).items()}


def small_cfg(D, build_encoder=True, **kw):
    e, d = RE.SMALL, R.SMALL
    enc = D.EncoderConfig(in_channels=3, latent_channels=e["latent_channels"], width_list=e["width_list"], depth_list=e["depth_list"],
                          block_type=list(e["block_type"]), norm="rms3d", act="silu", downsample_block_type="Conv", is_video=True,
                          temporal_downsample=e["temporal_downsample"])
    dec = D.DecoderConfig(in_channels=3, latent_channels=d["latent_channels"], width_list=d["width_list"], depth_list=d["depth_list"],
                          block_type=list(d["block_type"]), norm="rms3d", act="silu", upsample_block_type="InterpolateConv",
                          out_norm="rms3d", is_video=True, temporal_upsample=d["temporal_upsample"])
    return D.DCAEConfig(in_channels=3, latent_channels=e["latent_channels"], time_compression_ratio=4, spatial_compression_ratio=32,
                        encoder=enc, decoder=dec, build_encoder=build_encoder, **kw)


def small_model(D, dtype=torch.float32, **kw):
    m = D.DCAE(small_cfg(D, **kw)).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in small_state_dict().items()})
    return m


def restated(x, dtype=torch.float32, tiled=False):
    sd = {k: v.to(dtype) for k, v in R.make_state_dict(RE.enc_param_shapes(RE.SMALL)).items()}
    fn = lambda t: RE.encode(sd, RE.SMALL, t)  # noqa: E731
    with torch.no_grad():
        if not tiled:
            return fn(x.to(dtype))
        return RE.tiled_encode(fn, x.to(dtype), spatial=True, temporal=True, spatial_tile_size=128, temporal_tile_size=16,
                               spatial_tile_latent_size=4, temporal_tile_latent_size=4)


def golden_input(golden, tag):
    """a - c are stored; d is regenerated from its seed and checked against the stored subsample first"""
    if tag != "d":
        return torch.from_numpy(golden["x_" + tag])
    x = input_d()
    assert np.array_equal(x.flatten()[::SUB].numpy(), golden["x_d_sub"]), "the seeded generator no longer reproduces the input of d"
    return x


# ------------------------------------------------------------------------------------------------- restatement == reference
@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_restatement_matches_reference_golden(golden, tag):
    x = golden_input(golden, tag)
    assert tuple(x.shape) == SHAPES[tag]
    out = restated(x, tiled=tag == "d")
    want = torch.from_numpy(golden["z_" + tag])
    assert out.shape == want.shape
    assert rel_l2(out, want) <= 1e-5, (tag, rel_l2(out, want))


def test_golden_shapes(golden):
    assert tuple(golden["z_a"].shape) == (1, 32, 1, 2, 2) and tuple(golden["z_d"].shape) == (1, 32, 5, 5, 4)
    assert tuple(golden["z_b"].shape) == (1, 32, 1, 2, 1) and tuple(golden["z_c"].shape) == (1, 32, 1, 1, 2)


@needs_ref
def test_restatement_matches_live_reference():
    from tools.make_golden_dc_ae_enc import reference_dcae_full

    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        ref, _ = reference_dcae_full(RE.SMALL, R.SMALL)
        # (torch's CPU pixel_unshuffle refuses the reference's permuted view where the latent is one voxel per frame and T <= 4)
        for shape in ((1, 3, 4, 32, 64), (1, 3, 1, 64, 32), (2, 3, 2, 32, 64), (1, 3, 8, 32, 32)):
            x = torch.randn(shape, generator=g)
            assert rel_l2(restated(x), ref.encode(x)) <= 1e-5
        tiled, _ = reference_dcae_full(RE.SMALL, R.SMALL, use_spatial_tiling=True, use_temporal_tiling=True, **TILED)
        x = torch.randn(1, 3, 20, 160, 96, generator=g)
        assert rel_l2(restated(x, tiled=True), tiled.encode(x)) <= 1e-5


@needs_ref
def test_avg_shortcut_matches_live_reference_layer():
    from tools.make_golden_dc_ae import reference_module

    reference_module()
    from opensora.models.dc_ae.models.nn import ops

    g = torch.Generator().manual_seed(7)
    for cin, cout, factor, temporal, shape in ((32, 64, 2, False, (2, 3, 4, 6)), (64, 128, 2, True, (1, 4, 4, 2)),
                                               (64, 64, 2, True, (1, 1, 4, 4)), (64, 8, 1, False, (1, 3, 2, 2))):
        x = torch.randn(shape[0], cin, *shape[1:], generator=g)
        layer = ops.PixelUnshuffleChannelAveragingDownSampleLayer(cin, cout, factor, temporal)
        got, want = RE.avg_shortcut(x, cout, factor, temporal), layer(x)
        assert got.shape == want.shape and rel_l2(got, want) <= 1e-6     # the same elements; fp32 sums in another order


# ------------------------------------------------------------------------------------------------------------- state dict
def test_state_dict_keys_match_recorded_reference_keys(emu, golden):
    want = [str(k) for k in golden["keys"]]
    ours = small_model(emu).state_dict()
    assert list(ours) == want
    n_enc = sum(k.startswith("encoder.") for k in want)
    assert n_enc and all(k.startswith("encoder.") for k in want[:n_enc]) and all(k.startswith("decoder.") for k in want[n_enc:])
    shapes = dict(RE.enc_param_shapes(RE.SMALL))
    shapes.update(R.param_shapes(R.SMALL))
    assert list(shapes) == want
    assert {k: tuple(v.shape) for k, v in ours.items()} == {k: tuple(v) for k, v in shapes.items()}


def test_shipped_config_keys(emu):
    cfg = emu.dc_ae_f32("dc-ae-f32t4c128", None)
    cfg.build_encoder = True
    with torch.device("meta"):
        m = emu.DCAE(cfg)
    shapes = dict(RE.enc_param_shapes(RE.SHIPPED))
    shapes.update(R.param_shapes(R.SHIPPED))
    sd = m.state_dict()
    assert list(sd) == list(shapes)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v) for k, v in shapes.items()}
    assert tuple(sd["encoder.project_in.conv.weight"].shape) == (128, 3, 3, 3, 3)
    assert tuple(sd["encoder.stages.3.op_list.3.main.conv.weight"].shape) == (1024, 512, 3, 3, 3)
    assert m.encoder.stages[3].op_list[3].main.conv.stride == (2, 2, 2) and m.encoder.stages[0].op_list[2].main.conv.stride == (1, 2, 2)
    assert tuple(sd["encoder.project_out.main.op_list.0.conv.weight"].shape) == (128, 1024, 3, 3, 3)


@needs_ref
def test_shipped_config_keys_match_live_reference(emu):
    from tools.make_golden_dc_ae import reference_module

    D = reference_module()
    s = RE.SHIPPED
    with torch.device("meta"):
        ref = D.Encoder(D.EncoderConfig(in_channels=3, latent_channels=s["latent_channels"], width_list=s["width_list"],
                                        depth_list=s["depth_list"], block_type=list(s["block_type"]), norm="rms3d",
                                        downsample_block_type="Conv", is_video=True, temporal_downsample=s["temporal_downsample"]))
    a = {"encoder." + k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert a == {k: tuple(v) for k, v in RE.enc_param_shapes(s).items()} and list(a) == list(RE.enc_param_shapes(s))


def test_default_model_has_no_encoder_and_still_refuses(emu):
    assert emu.DCAEConfig().build_encoder is False
    assert list(emu.DCAEConfig.__dataclass_fields__)[-1] == "build_encoder"
    m = emu.DCAE(small_cfg(emu, build_encoder=False))
    assert not hasattr(m, "encoder") and not any(k.startswith("encoder.") for k in m.state_dict())
    for fn in (m.encode, m.forward, m._encode):
        with pytest.raises(NotImplementedError, match="DECODER") as e:
            fn(torch.zeros(1, 3, 4, 32, 32))
        assert "build_encoder" in str(e.value)
    m.load_state_dict(small_state_dict())                     # strict: passes because encoder.* is dropped
    assert not any(k.startswith("encoder.") for k in m.state_dict())


def test_encoder_keys_load_strictly(emu):
    m = emu.DCAE(small_cfg(emu))
    sd = small_state_dict()
    m.load_state_dict(sd)
    got = m.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    short = dict(sd)
    short.pop("encoder.project_in.conv.bias")
    with pytest.raises(RuntimeError, match="encoder.project_in.conv.bias"):
        m.load_state_dict(short)
    extra = dict(sd)
    extra["encoder.stages.0.op_list.1.main.norm.weight"] = torch.zeros(32)
    with pytest.raises(RuntimeError, match="encoder.stages.0.op_list.1.main.norm.weight"):
        m.load_state_dict(extra)
    with pytest.raises(RuntimeError, match="encoder"):
        m.load_state_dict({k: v for k, v in sd.items() if k.startswith("decoder.")})


def test_load_state_dict_drops_cached_plans(emu, golden):
    m = small_model(emu, BF)
    x = torch.from_numpy(golden["x_b"]).to(BF)
    with torch.no_grad():
        z0 = m.encode(x)
        sd = small_state_dict()
        sd["encoder.project_out.main.op_list.0.conv.bias"] = sd["encoder.project_out.main.op_list.0.conv.bias"] + 1.0
        m.load_state_dict(sd)
        z1 = m.encode(x)
    assert float((z1.float() - z0.float()).min()) > 0.5        # the new bias (+1 on every latent channel) took effect


def test_checkpoint_file_with_both_halves_loads(emu, tmp_path):
    from safetensors.torch import save_file

    from open_sora_amd.ckpt import load_checkpoint

    sd = {k: v.contiguous() for k, v in small_state_dict().items()}
    path = str(tmp_path / "dcae_full.safetensors")
    save_file(sd, path)
    m = load_checkpoint(emu.DCAE(small_cfg(emu)), path, device_map="cpu")
    got = m.state_dict()
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


# ----------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("field,value,match", [
    ("is_video", False, "2-D image encoder"),
    ("downsample_block_type", "ConvPixelUnshuffle", "downsample_block_type 'ConvPixelUnshuffle'"),
    ("downsample_shortcut", None, "shortcuts None"),
    ("out_shortcut", None, "shortcuts 'averaging' / None"),
    ("out_norm", "rms3d", "project_out norm / act 'rms3d'"),
    ("out_act", "relu", "project_out norm / act None / 'relu'"),
    ("double_latent", True, "double_latent"),
    ("downsample_match_channel", False, "downsample_match_channel"),
    ("depth_list", (0, 1, 1, 1, 1, 1), "depth_list\\[0\\] == 0"),
    ("depth_list", (1, 1, 0, 1, 1, 1), "an empty stage 2"),
    ("block_type", ["ResBlock"] * 5 + ["EViT_GLU"], "block_type 'EViT_GLU'"),
    ("norm", "bn2d", "norm 'bn2d'"),
    ("act", "relu6", "activation 'relu6'"),
    ("width_list", (32, 32, 64, 64, 64, 96), "width 96"),
    ("width_list", (16, 32, 64, 64, 64, 64), "width 16"),
    ("in_channels", 12, "in_channels 12"),
    ("latent_channels", 12, "latent_channels 12"),
    ("latent_channels", 24, "latent_channels 24"),
    ("width_list", (32, 32, 64, 64, 64, 512), "downsample 64 -> 512"),
])
def test_unsupported_encoder_configurations_are_refused_at_construction(emu, field, value, match):
    cfg = small_cfg(emu)
    setattr(cfg.encoder, field, value)
    with pytest.raises(ValueError, match=match):
        emu.DCAE(cfg)
    cfg.build_encoder = False                                 # the encoder's configuration is not looked at without it
    emu.DCAE(cfg)


def test_in_channels_up_to_8_are_padded_and_8_2j_taken(emu):
    for c in (1, 3, 8, 16):
        cfg = small_cfg(emu)
        cfg.encoder.in_channels = c
        m = emu.DCAE(cfg)
        assert tuple(m.encoder.project_in.conv.weight.shape) == (32, c, 3, 3, 3)


# ------------------------------------------------------------------------------------------------- shape validation
class _Counting:
    """a kernel table that counts every call and runs none"""

    def __init__(self):
        self.calls = 0

    def __getattr__(self, name):
        def op(*a, **k):
            self.calls += 1
            raise AssertionError(f"{name} was launched")
        return op


@pytest.mark.parametrize("shape,match", [
    ((1, 3, 3, 32, 32), "T must be 1 or even"),
    ((1, 3, 6, 32, 32), "T must be 1 or even"),              # 6 -> 3 at the second temporal stage
    ((2, 3, 5, 64, 32), "T must be 1 or even"),
    ((1, 3, 4, 48, 32), "multiples of 32"),
    ((1, 3, 4, 32, 33), "multiples of 32"),
    ((1, 4, 4, 32, 32), "3 channels"),
])
def test_bad_shapes_raise_before_anything_is_launched(emu, shape, match):
    from open_sora_amd import mmdit

    m = small_model(emu, BF)
    table = _Counting()
    mmdit.set_ops_for_testing(table)
    try:
        with pytest.raises(ValueError, match=match) as e:
            m.encode(torch.zeros(shape, dtype=BF))
        assert str(tuple(shape)) in str(e.value)
    finally:
        mmdit.set_ops_for_testing(cpu_ops_dc_ae_enc)
    assert table.calls == 0


@pytest.mark.parametrize("T", [1, 2, 4, 8, 12])
def test_legal_frame_counts(emu, T):
    m = small_model(emu, BF)
    m._check_encode_shape(torch.zeros(1, 3, T, 32, 32))


# --------------------------------------------------------------------------------------------------------------- tile loop
def _stub(x):
    """a deterministic `_encode`: 32 channels from the 3, strided 4 x 32 x 32 (bf16-representable)"""
    return x.repeat(1, 11, 1, 1, 1)[:, :32, ::4, ::32, ::32].contiguous()


TILE_CASES = [
    # pixel shape, spatial, temporal tiling, pixel tile sizes (the latent tile sizes follow from the config)
    ((1, 3, 20, 160, 128), True, True, 128, 16),    # the golden's case d: short last tiles on T, H and W
    ((1, 3, 28, 128, 288), True, True, 128, 16),    # a last temporal tile of 4 frames; H fits in one tile
    ((1, 3, 8, 320, 320), True, False, 128, 16),    # spatial only, 4 x 4 tiles, the last of one latent row / column
    ((1, 3, 52, 96, 96), False, True, 128, 16),     # temporal only
    ((1, 3, 36, 288, 288), True, True, 256, 32),    # the shipped tile sizes
    ((1, 3, 16, 128, 128), True, True, 128, 16),    # nothing exceeds a tile: no tiling
]


@pytest.mark.parametrize("shape,sp,tp,sts,tts", TILE_CASES)
def test_tile_loop_matches_restatement(emu, monkeypatch, shape, sp, tp, sts, tts):
    m = small_model(emu, use_spatial_tiling=sp, use_temporal_tiling=tp, spatial_tile_size=sts, temporal_tile_size=tts)
    calls = []

    def stub(x):
        calls.append(tuple(x.shape))
        return _stub(x)

    monkeypatch.setattr(m, "_encode", stub)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(BF)
    out = m.encode(x.clone())
    want_calls = []

    def stub32(t):
        want_calls.append(tuple(t.shape))
        return _stub(t)

    want = RE.tiled_encode(stub32, x.float(), spatial=sp, temporal=tp, spatial_tile_size=sts, temporal_tile_size=tts,
                           spatial_tile_latent_size=sts // 32, temporal_tile_latent_size=tts // 4)
    assert calls == want_calls                     # the same tiles, in the same order, short last tiles included
    assert out.dtype == BF and out.shape == want.shape
    # the cross-fades run in f32 with one bf16 rounding per fade (two where a vertical and a horizontal fade overlap)
    assert rel_l2(out, want) <= 2 * 2.0 ** -9, rel_l2(out, want)


@needs_ref
@pytest.mark.parametrize("shape,sp,tp,sts,tts", TILE_CASES)
def test_tile_loop_matches_live_reference(emu, monkeypatch, shape, sp, tp, sts, tts):
    from tools.make_golden_dc_ae_enc import reference_dcae_full

    ref, _ = reference_dcae_full(RE.SMALL, R.SMALL, use_spatial_tiling=sp, use_temporal_tiling=tp, spatial_tile_size=sts,
                                 temporal_tile_size=tts)
    m = small_model(emu, use_spatial_tiling=sp, use_temporal_tiling=tp, spatial_tile_size=sts, temporal_tile_size=tts)
    ours_calls, ref_calls = [], []
    monkeypatch.setattr(m, "_encode", lambda t: (ours_calls.append(tuple(t.shape)), _stub(t))[1])
    monkeypatch.setattr(ref, "_encode", lambda t: (ref_calls.append(tuple(t.shape)), _stub(t))[1])
    x = torch.randn(shape, generator=torch.Generator().manual_seed(2)).to(BF)
    out, want = m.encode(x.clone()), ref.encode(x.float())
    assert ours_calls == ref_calls and out.shape == want.shape
    assert rel_l2(out, want) <= 2 * 2.0 ** -9


# ------------------------------------------------------------------------------- the encoder through the emulated kernels
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_emulated_encode_matches_golden(emu, golden, tag):
    x = golden_input(golden, tag)
    with torch.no_grad():
        out = small_model(emu, BF).encode(x.to(BF))
    assert out.dtype == BF
    ref_bf16 = finite_retry(lambda: restated(x, BF))
    assert_parity(out, torch.from_numpy(golden["z_" + tag]), ref_bf16, f"emulated encode {tag}")


def test_emulated_tiled_encode_matches_golden(emu, golden):
    x = golden_input(golden, "d")
    with torch.no_grad():
        m = small_model(emu, BF, use_spatial_tiling=True, use_temporal_tiling=True, **TILED)
        out = m.encode(x.to(BF))
    assert tuple(out.shape) == (1, 32, 5, 5, 4)
    ref_bf16 = finite_retry(lambda: restated(x, BF, tiled=True))
    assert_parity(out, torch.from_numpy(golden["z_d"]), ref_bf16, "emulated tiled encode d")


def test_emulated_batch_and_scaling_factor(emu, golden):
    """a batch is a per-sample loop; the latent is divided by scaling_factor; the result comes back in x's dtype"""
    x = torch.cat([torch.from_numpy(golden["x_a"]), torch.from_numpy(golden["x_a"]).flip(2)])
    m = small_model(emu, BF)
    with torch.no_grad():
        z = m.encode(x)
        assert z.dtype == torch.float32 and tuple(z.shape) == (2, 32, 1, 2, 2)
        assert torch.equal(z[:1], m.encode(x[:1])) and torch.equal(z[1:], m.encode(x[1:]))
        m.scaling_factor = 0.5
        assert torch.equal(m.encode(x), z / 0.5)


def test_emulated_encode_runs_only_kernel_table_ops_between_the_boundaries(emu, golden, monkeypatch):
    """run_encoder gets NDHWC bf16 with 8 channels (3 live) and hands back NDHWC bf16"""
    seen = {}
    plain = emu.run_encoder

    def spy(enc, x):
        seen["in"] = (tuple(x.shape), x.dtype, float(x[..., 3:].abs().sum()))
        z = plain(enc, x)
        seen["out"] = (tuple(z.shape), z.dtype)
        return z

    monkeypatch.setattr(emu, "run_encoder", spy)
    with torch.no_grad():
        small_model(emu, BF).encode(torch.from_numpy(golden["x_a"]))
    assert seen["in"] == ((1, 4, 64, 64, 8), BF, 0.0) and seen["out"] == ((1, 1, 2, 2, 32), BF)


def test_forward_returns_dec_none_z(emu):
    x = torch.randn(1, 3, 8, 32, 32, generator=torch.Generator().manual_seed(9))
    m = small_model(emu, BF)
    with torch.no_grad():
        dec, mid, z = m(x)
        assert mid is None
        assert dec.shape == x.shape and dec.dtype == x.dtype
        assert tuple(z.shape) == (1, 32, 2, 1, 1) and z.dtype == BF
        assert torch.equal(z, m.encode(x.to(BF)))
        assert torch.equal(dec, m.decode(z).to(x.dtype))


def test_training_mode_is_refused(emu):
    m = small_model(emu, BF)
    m.cfg.is_training = True
    with pytest.raises(ValueError, match="is_training"):
        m.encode(torch.zeros(1, 3, 4, 32, 32))


# --------------------------------------------------------------------------------------------------------------- factory
def test_factory_with_encoder_mirrors_dc_ae(emu):
    assert list(inspect.signature(emu.DC_AE_with_encoder).parameters) == list(inspect.signature(emu.DC_AE).parameters)
    a, b = inspect.signature(emu.DC_AE_with_encoder), inspect.signature(emu.DC_AE)
    assert [p.default for p in a.parameters.values()] == [p.default for p in b.parameters.values()]
    m = emu.DC_AE_with_encoder("dc-ae-f32t4c128", device_map="meta", from_scratch=True, use_spatial_tiling=True, spatial_tile_size=128,
                               scaling_factor=0.5)
    assert m.cfg.build_encoder and isinstance(m.encoder, emu.Encoder) and list(m._modules)[:2] == ["encoder", "decoder"]
    assert m.use_spatial_tiling and m.spatial_tile_size == 128 and m.scaling_factor == 0.5
    plain = emu.DC_AE("dc-ae-f32t4c128", device_map="meta", from_scratch=True)
    assert not plain.cfg.build_encoder and not hasattr(plain, "encoder")
    with pytest.raises(ValueError, match="from_pretrained"):
        emu.DC_AE_with_encoder("dc-ae-f32t4c128", device_map="meta")


# ------------------------------------------------------------------------------------------------------- the emulation itself
def test_emulated_ops_match_torch():
    """conv3d_zp_strided_ref == F.conv3d(stride) on the padded input; unshuffle_avg_ref == the restatement's avg_shortcut"""
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(4)
    for (B, T, H, W), st in (((2, 5, 7, 9), 2), ((1, 1, 4, 6), 2), ((1, 4, 6, 5), 1), ((2, 2, 4, 4), 2)):
        x = torch.randn(B, T, H, W, 16, generator=g)
        w = torch.randn(24, 16, 3, 3, 3, generator=g)
        b = torch.randn(24, generator=g)
        wk = torch.zeros(24, 448)
        wk[:, :432] = w.permute(0, 2, 3, 4, 1).reshape(24, 432)
        want = F.conv3d(F.pad(x.permute(0, 4, 1, 2, 3), (1,) * 6), w, b, stride=(st, 2, 2)).permute(0, 2, 3, 4, 1)
        got = cpu_ops_dc_ae_enc.conv3d_zp_strided_ref(x, wk, b, st, 2, None, dtype=torch.float64)
        assert got.shape == want.shape and rel_l2(got, want) <= 1e-6
    for cin, cout, ft, fhw, shape in ((32, 64, 1, 2, (2, 3, 4, 6)), (64, 128, 2, 2, (1, 4, 4, 2)), (64, 8, 1, 1, (1, 3, 2, 2)),
                                      (32, 32, 2, 2, (2, 2, 2, 4))):
        x = torch.randn(shape[0], *shape[1:], cin, generator=g)
        want = RE.avg_shortcut(x.permute(0, 4, 1, 2, 3).double(), cout, fhw, ft == 2).permute(0, 2, 3, 4, 1)
        got = cpu_ops_dc_ae_enc.unshuffle_avg_ref(x, cout, ft, fhw, dtype=torch.float64)
        assert got.shape == want.shape and rel_l2(got, want) <= 1e-12
