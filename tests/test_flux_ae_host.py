"""CPU: host side of the Flux 2-D autoencoder (open_sora_amd.flux_ae) and of the distilled image sampler
(sampling.DistilledDenoiser), driven through the CPU emulation of the kernels' semantics (tests/cpu_ops_flux.py) and compared
with the reference's own modules (oracle.ref_loader; those tests skip where the reference tree is absent), and the plain-torch
restatement the GPU tests take as truth (tests/flux_ae_restatement.py) pinned to the reference and to its committed output.
The kernels themselves are checked on the GPU by tests/test_gpu_flux_ae.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import configs, ref_loader
from tests import cpu_ops_flux
from tests import flux_ae_restatement as R
from tests.cpu_ops_flux import conv2d_ref
from tests.util import assert_parity, finite_retry, torch_inputs, torch_params

BF = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flux_ae_small.npz")
needs_ref = pytest.mark.skipif(not ref_loader.available(), reason="needs the reference tree (oracle.ref_loader)")


@pytest.fixture()
def emu(hip_lib):
    from open_sora_amd import flux_ae, mmdit

    mmdit.set_ops_for_testing(cpu_ops_flux)
    yield flux_ae
    mmdit.set_ops_for_testing(hip_lib)


def _ref_module(cfg, dtype=torch.float32):
    ref_loader.install()
    from opensora.models.vae.autoencoder_2d import AutoEncoderFlux

    return AutoEncoderFlux(from_pretrained=None, device_map="cpu", torch_dtype=dtype, **cfg)


# ------------------------------------------------------------------------------------------------------------- state dict
@needs_ref
@pytest.mark.parametrize("cfg", [{}, R.SMALL], ids=["default", "small"])
def test_state_dict_keys_and_shapes_match_reference(emu, cfg):
    ref = _ref_module(cfg)
    ours = emu.AutoEncoderFlux(from_pretrained=None, device_map="cpu", torch_dtype=torch.float32, **cfg)
    a = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    b = {k: tuple(v.shape) for k, v in ours.state_dict().items()}
    assert a == b
    if not cfg:
        assert sum(v.numel() for v in ours.state_dict().values()) == 83_819_683


def test_checkpoint_round_trip_loads_strictly(emu, tmp_path):
    """a safetensors file written from the module's own state dict (the flux1-dev-ae.safetensors key set) loads through
    open_sora_amd.ckpt.load_checkpoint with every key matched"""
    from safetensors.torch import save_file

    src = emu.AutoEncoderFlux(from_pretrained=None, device_map="cpu", torch_dtype=torch.float32, **R.SMALL)
    sd = R.make_state_dict(src)
    path = str(tmp_path / "ae.safetensors")
    save_file({k: v.contiguous() for k, v in sd.items()}, path)
    m = emu.AutoEncoderFlux(from_pretrained=path, device_map="cpu", torch_dtype=torch.float32, **R.SMALL)
    got = m.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


def test_unsupported_channel_widths_are_refused(emu):
    """osk_conv2d_nhwc_bf16 takes Cin = 8 * 2^j: a width the kernel cannot take is refused at construction, not at the first
    decode"""
    with pytest.raises(ValueError, match="8 \\* 2\\^j"):
        emu.AutoEncoderFlux(from_pretrained=None, device_map="cpu", torch_dtype=torch.float32, ch=96, ch_mult=[1, 2])


# --------------------------------------------------------------------------------------------------------- conv emulation
# (name, Cin, Cout, H, W, ksize, stride, up, res, torch form: padding or "down")
_MODES = [
    ("pad1", 16, 24, 7, 9, 3, 1, False, False, 1),
    ("pad1_res", 16, 8, 6, 5, 3, 1, False, True, 1),
    ("up", 8, 16, 4, 5, 3, 1, True, False, 1),
    ("down", 16, 16, 9, 8, 3, 2, False, False, "down"),
    ("1x1", 32, 16, 5, 6, 1, 1, False, False, 0),
    ("cout3", 32, 3, 6, 7, 3, 1, False, False, 1),
    ("cin3_pad8", 3, 16, 6, 6, 3, 1, False, False, 1),
]


@pytest.mark.parametrize("mode", _MODES, ids=[m[0] for m in _MODES])
def test_conv2d_emulation_matches_torch_conv_f64(emu, mode):
    name, Cin, Cout, H, W, k, s, up, with_res, form = mode
    g = torch.Generator().manual_seed(5)
    conv = torch.nn.Conv2d(Cin, Cout, k, stride=s, padding=0 if form == "down" else form).double()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g, dtype=torch.float64).to(BF))
        conv.bias.copy_(torch.randn(Cout, generator=g, dtype=torch.float64).float())
    plan = emu._Conv2dPlan(conv)
    x = torch.randn(1, Cin, H, W, generator=g).to(BF).double()
    xin = F.interpolate(x, scale_factor=2.0, mode="nearest") if up else x
    with torch.no_grad():
        want = conv(F.pad(xin, (0, 1, 0, 1)) if form == "down" else xin)
    Ho, Wo = want.shape[2:]
    assert (Ho, Wo) == emu.conv2d_out_dims(H, W, k, s, plan.pad, up, 1 if form == "down" else None)
    res = torch.randn(1, Ho, Wo, Cout, generator=g).to(BF) if with_res else None
    if res is not None:
        want = want + res.double().permute(0, 3, 1, 2)
    want = want.permute(0, 2, 3, 1)
    xn = torch.zeros(1, H, W, plan.cin_p, dtype=BF)
    xn[..., :Cin] = x.permute(0, 2, 3, 1).to(BF)
    got = conv2d_ref(xn, plan.w, plan.b, k, s, plan.pad, up, res, Ho, Wo, dtype=torch.float64)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12), name
    out = torch.empty(1, Ho, Wo, Cout, dtype=BF)
    cpu_ops_flux.conv2d(xn, plan.w, plan.b, out, k, s, plan.pad, up, res)
    assert float((out.double() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())


@needs_ref
@pytest.mark.parametrize("cfg", [R.SMALL, R.SHIPPED], ids=["small", "shipped_widths"])
def test_package_decode_encode_on_emulation_vs_reference(emu, cfg):
    lat = 8
    ref = _ref_module(cfg)
    sd = R.make_state_dict(ref)
    ref.load_state_dict(sd, strict=True)
    ref.sample = False
    ours = emu.AutoEncoderFlux(from_pretrained=None, device_map="cpu", torch_dtype=BF, **cfg)
    ours.load_state_dict(sd, strict=True)
    ours.sample = False
    up = 2 ** (len(cfg["ch_mult"]) - 1)
    g = torch.Generator().manual_seed(1)
    z = torch.randn(1, 16, 1, lat, lat, generator=g).to(BF).float()
    x = (0.5 * torch.randn(1, 3, 1, lat * up, lat * up, generator=g)).to(BF).float()
    with torch.inference_mode():
        d_t, e_t = ref.decode(z), ref.encode(x)
        refb = _ref_module(cfg, BF)
        refb.load_state_dict(sd, strict=True)
        refb.sample = False
        d_r = finite_retry(lambda: refb.decode(z.to(BF)))
        e_r = finite_retry(lambda: refb.encode(x.to(BF)))
        d, e = ours.decode(z.to(BF)), ours.encode(x.to(BF))
    assert d.shape == d_t.shape and e.shape == e_t.shape and d.dtype == BF
    assert_parity(d, d_t, d_r, "flux_ae decode (CPU emulation) vs reference")
    assert_parity(e, e_t, e_r, "flux_ae encode (CPU emulation) vs reference")


# ------------------------------------------------------------------------------------------------------ restatement pins
@needs_ref
@pytest.mark.parametrize("cfg,B,T,h,w", [(R.SMALL, 2, 2, 6, 10), (R.SHIPPED, 1, 1, 6, 10)], ids=["small", "shipped_widths"])
def test_restatement_equals_reference_module(cfg, B, T, h, w):
    """the plain-torch restatement (the GPU tests' truth) is the reference module to fp32 rounding: decode and encode, at the small
    geometry and at the shipped widths"""
    ref = _ref_module(cfg)
    sd = R.make_state_dict(ref)
    ref.load_state_dict(sd, strict=True)
    ref.sample = False
    up = 2 ** (len(cfg["ch_mult"]) - 1)
    g = torch.Generator().manual_seed(2)
    z = torch.randn(B, 16, T, h, w, generator=g)
    x = 0.5 * torch.randn(B, 3, T, h * up, w * up, generator=g)
    with torch.inference_mode():
        d_t, e_t = ref.decode(z), ref.encode(x)
        d, e = R.decode(sd, cfg, z), R.encode_mode(sd, cfg, x)
    assert d.shape == d_t.shape and e.shape == e_t.shape
    assert float((d - d_t).abs().max()) <= 1e-5 * float(d_t.abs().max())
    assert float((e - e_t).abs().max()) <= 1e-5 * float(e_t.abs().max())


def test_restatement_reproduces_reference_golden(emu):
    """no reference tree needed: the restatement on the committed fixture's inputs gives the reference's recorded outputs"""
    gold = np.load(GOLDEN)
    sd = R.make_state_dict(emu.AutoEncoderFlux(from_pretrained=None, device_map="cpu", torch_dtype=torch.float32, **R.SMALL))
    with torch.inference_mode():
        d = R.decode(sd, R.SMALL, torch.from_numpy(gold["z"]))
        e = R.encode_mode(sd, R.SMALL, torch.from_numpy(gold["x"]))
    dg, eg = torch.from_numpy(gold["dec"]), torch.from_numpy(gold["enc"])
    assert d.shape == dg.shape and e.shape == eg.shape
    assert float((d - dg).abs().max()) <= 1e-5 * float(dg.abs().max())
    assert float((e - eg).abs().max()) <= 1e-5 * float(eg.abs().max())


# -------------------------------------------------------------------------------------------------------- distilled sampler
_DCFG = dict(configs.GOLDEN["hd64_liger_split"][0], cond_embed=False)   # guidance_embed=True, cond_embed=False: flux-dev's flags


def _tiny_flux():
    from open_sora_amd import mmdit

    m = mmdit.Flux(device_map="cpu", torch_dtype=BF, **_DCFG)
    m.load_state_dict(torch_params(_DCFG, dtype=BF), strict=True)
    return m


@needs_ref
def test_distilled_denoiser_matches_reference_bit_for_bit(emu):
    from oracle.make_golden_refchecks import ref_namespace
    from open_sora_amd import sampling

    ns = ref_namespace()
    model = _tiny_flux()
    inp = torch_inputs(_DCFG, 1, 1, 4, 6, 24, dtype=BF)
    inp.pop("timesteps"), inp.pop("guidance")
    ts = sampling.get_schedule(4, 24, 1)
    with torch.inference_mode():
        theirs = ns["DistilledDenoiser"]().denoise(model, **dict(inp, timesteps=ts, guidance=3.5))
        ours = sampling.DistilledDenoiser().denoise(model, **dict(inp, timesteps=ts, guidance=3.5))
    assert ours.dtype == theirs.dtype == BF and torch.equal(ours, theirs)
    assert sampling.DistilledDenoiser().prepare_guidance(["a", "b"], {}, "cpu", BF, neg=None, guidance_img=3.0) == (["a", "b"], {})
    assert isinstance(sampling.SamplingMethodDict["distill"], sampling.DistilledDenoiser)
    assert isinstance(sampling.SamplingMethodDict["i2v"], sampling.I2VDenoiser)


@needs_ref
def test_reference_prepare_api_drives_flux_and_flux_ae(emu):
    """the reference's own prepare_api with method DISTILLED and one frame (the image stage of t2i2v) driving mmdit.Flux as the
    image model and flux_ae.AutoEncoderFlux as its autoencoder; its image equals the package's own composition
    noise -> DistilledDenoiser -> unpack -> decode"""
    from oracle.make_golden_refchecks import ref_namespace
    from open_sora_amd import sampling
    from tests.ref_cases import ClipStub, T5Stub

    ns = ref_namespace()
    model = _tiny_flux()
    ae = emu.AutoEncoderFlux(from_pretrained=None, device_map="cpu", torch_dtype=BF, **R.SMALL)
    ae.load_state_dict(R.make_state_dict(ae), strict=True)
    kw = dict(height=64, width=96, num_frames=1, num_steps=3, guidance=3.5, seed=9, is_causal_vae=True, temporal_reduction=4,
              method="distill")
    opt = ns["sanitize_sampling_option"](ns["SamplingOption"](**kw))
    with torch.inference_mode():
        theirs = ns["prepare_api"](model, ae, T5Stub(), ClipStub(), {})(opt, cond_type="t2v", text=["a cat"], channel=64)
        z = sampling.get_noise(1, 64, 96, 1, torch.device("cpu"), BF, 9, patch_size=2, channel=16)
        Hl, Wl = z.shape[-2:]
        txt, y_vec = T5Stub()(["a cat"], added_tokens=(Hl // 2) * (Wl // 2)).to(BF), ClipStub()(["a cat"]).to(BF)
        img_ids, txt_ids = sampling.prepare_ids(1, 1, Hl, Wl, txt.shape[1], "cpu", BF)
        x = sampling.DistilledDenoiser().denoise(model, img=sampling.pack(z), timesteps=sampling.get_schedule(3, (Hl // 2) * (Wl // 2), 1),
                                                 guidance=3.5, img_ids=img_ids, txt=txt, txt_ids=txt_ids, y_vec=y_vec)
        ours = ae.decode(sampling.unpack(x, 64, 96, 1))[:, :, :1]
    assert theirs.shape == ours.shape == (1, 3, 1, Hl * 4, Wl * 4)
    assert torch.equal(ours, theirs)


# ------------------------------------------------------------------------------------------------------------ bad arguments
def test_conv2d_entry_rejects_bad_arguments(hip_lib):
    lib = hip_lib.lib
    P = 0x100000   # 16-byte aligned fake device pointers: the argument checks run before any HIP call, nothing is launched

    def call(Cin=128, ksize=3, stride=1, pad=1, up=0, Ho=8, Wo=8, wrs=1152, gn=None, G=0, x=P):
        return lib.osk_conv2d_nhwc_bf16(x, 1, 8, 8, Cin, P, wrs, None, 128, ksize, stride, pad, up, None, P, Ho, Wo, gn, G, None)

    assert call(ksize=2) < 0
    assert call(Cin=12) < 0                    # not a multiple of 8
    assert call(Cin=24) < 0                    # not 8 * 2^j
    assert call(stride=3) < 0
    assert call(pad=3) < 0
    assert call(up=2) < 0
    assert call(Ho=10) < 0                     # the last output row's window starts beyond the image
    assert call(wrs=1088) < 0                  # weight row shorter than round_up(9 * Cin, 64)
    assert call(x=None) < 0
    assert call(x=P + 2) < 0                   # misaligned activation
    assert call(gn=P, G=32) == hip_lib.OSK_EUNSUPPORTED   # no fused-statistics epilogue: declined, nothing launched
