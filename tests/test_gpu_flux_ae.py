"""GPU: the Flux 2-D autoencoder (open_sora_amd.flux_ae) and the distilled image sampler (sampling.DistilledDenoiser) on the MI355X.

- osk_conv2d_nhwc_bf16 against an f64 restatement on every layer class of the shipped encoder and decoder, the zero-padded
  border rows / columns judged separately from the interior;
- the shipped-width decode at the default t2i2v image (latent 16 x 72 x 128 -> 576 x 1024) and the shipped encoder at 256 x 256
  against the plain-torch fp32 restatement (tests/flux_ae_restatement.py), with the same restatement in bf16 as the
  reference-precision comparator;
- the small-geometry decode / encode against the committed fixture the reference itself produced;
- three distilled steps of a tiny flux-style denoiser against an fp32 loop around the oracle forward, the hipGraph replay bit for
  bit against the eager loop, and the image stage (denoise -> unpack -> decode) against its CPU composition."""
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import configs, sampling_oracle as SO
from tests import cpu_ops_flux
from tests import flux_ae_restatement as R
from tests.cpu_ops_flux import conv2d_ref
from tests.util import assert_parity, torch_inputs, torch_params

BF = torch.bfloat16
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flux_ae_small.npz")

# (name, Cin, Cout, H, W (source), ksize, stride, pad, pad_far, up, res, bias)
CONV_CASES = [
    ("dec_conv_in_16_512", 16, 512, 72, 128, 3, 1, 1, 1, False, False, True),
    ("512_512_res", 512, 512, 72, 128, 3, 1, 1, 1, False, True, True),
    ("512_512_up", 512, 512, 36, 64, 3, 1, 1, 1, True, False, True),
    ("512_256_odd", 512, 256, 23, 37, 3, 1, 1, 1, False, False, True),
    ("256_256_up_res", 256, 256, 12, 21, 3, 1, 1, 1, True, True, True),
    ("256_128", 256, 128, 24, 42, 3, 1, 1, 1, False, False, True),
    ("128_128_res_nobias", 128, 128, 72, 128, 3, 1, 1, 1, False, True, False),
    ("128_128_up_odd", 128, 128, 12, 19, 3, 1, 1, 1, True, False, True),
    ("dec_conv_out_128_3", 128, 3, 72, 128, 3, 1, 1, 1, False, False, True),
    ("enc_conv_in_3p8_128", 3, 128, 72, 128, 3, 1, 1, 1, False, False, True),
    ("enc_conv_out_512_32", 512, 32, 24, 42, 3, 1, 1, 1, False, False, True),
    ("down_128", 128, 128, 48, 84, 3, 2, 0, 1, False, False, True),
    ("down_256", 256, 256, 24, 42, 3, 2, 0, 1, False, False, True),
    ("down_512_odd", 512, 512, 23, 37, 3, 2, 0, 1, False, False, True),
    ("nin_512_256", 512, 256, 24, 42, 1, 1, 0, 0, False, False, True),
]


@pytest.fixture()
def flux_ae(hip_lib):
    from open_sora_amd import flux_ae, mmdit

    mmdit.set_ops_for_testing(hip_lib)
    torch.cuda.set_device(0)
    return flux_ae


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv2d_kernel_vs_f64(flux_ae, case):
    name, Cin, Cout, H, W, k, s, pad, pad_far, up, with_res, with_bias = case
    g = _gen(zlib.crc32(name.encode()) % 1000)
    conv = torch.nn.Conv2d(Cin, Cout, k, stride=s, padding=pad, bias=with_bias).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g, device=DEV) / (Cin * k * k) ** 0.5)
        if with_bias:
            conv.bias.copy_(0.1 * torch.randn(Cout, generator=g, device=DEV))
    plan = flux_ae._Conv2dPlan(conv)
    x = torch.zeros(1, H, W, plan.cin_p, dtype=BF, device=DEV)
    x[..., :Cin] = torch.randn(1, H, W, Cin, generator=g, device=DEV).to(BF)
    Ho, Wo = flux_ae.conv2d_out_dims(H, W, k, s, pad, up, pad_far)
    res = torch.randn(1, Ho, Wo, Cout, generator=g, device=DEV).to(BF) if with_res else None
    out = torch.full((1, Ho, Wo, Cout), float("nan"), dtype=BF, device=DEV)
    from open_sora_amd import _C

    _C.conv2d(x, plan.w, plan.b, out, k, s, pad, up, res)
    torch.cuda.synchronize()
    y = conv2d_ref(x, plan.w, plan.b, k, s, pad, up, res, Ho, Wo, dtype=torch.float64)
    err = (out.double() - y).abs()
    bound = 2.0 ** -8 * y.abs() + 1e-4 * float(y.abs().max())
    border = torch.zeros(Ho, Wo, dtype=torch.bool, device=DEV)
    border[:4], border[-4:], border[:, :4], border[:, -4:] = True, True, True, True
    border = border[None, :, :, None].expand_as(err)
    e_b, e_i = float(err[border].max()), float(err[~border].max()) if (~border).any() else 0.0
    print(f"{name}: max-abs border {e_b:.3e} interior {e_i:.3e} (max |y| {float(y.abs().max()):.3e})")
    assert torch.isfinite(out.float()).all(), name
    assert bool((err[border] <= bound[border]).all()), f"{name}: border rows / columns off by up to {e_b:.3e}"
    assert bool((err[~border] <= bound[~border]).all()), f"{name}: interior off by up to {e_i:.3e}"


@pytest.mark.gpu
def test_conv2d_gn_epilogue_declined_without_launch(flux_ae, hip_lib):
    """the fused-statistics argument is refused with OSK_EUNSUPPORTED: nothing is written, the statistics stay zero"""
    conv = torch.nn.Conv2d(128, 128, 3, padding=1).to(DEV)
    plan = flux_ae._Conv2dPlan(conv)
    x = torch.randn(1, 16, 16, 128, device=DEV).to(BF)
    out = torch.zeros(1, 16, 16, 128, dtype=BF, device=DEV)
    sums = torch.zeros(1, 32, 2, dtype=torch.float64, device=DEV)
    rc = hip_lib.lib.osk_conv2d_nhwc_bf16(x.data_ptr(), 1, 16, 16, 128, plan.w.data_ptr(), plan.w.stride(0), plan.b.data_ptr(), 128,
                                          3, 1, 1, 0, None, out.data_ptr(), 16, 16, sums.data_ptr(), 32, hip_lib._stream())
    torch.cuda.synchronize()
    assert rc == hip_lib.OSK_EUNSUPPORTED and float(out.float().abs().sum()) == 0.0 and float(sums.abs().sum()) == 0.0


_MODELS: dict = {}


def _model(flux_ae, cfg, dtype=BF):
    """(model on the GPU, its f32 CPU state dict), made once per geometry (the shipped one has 84 M parameters)"""
    key = (str(cfg), dtype)
    if key not in _MODELS:
        m = flux_ae.AutoEncoderFlux(from_pretrained=None, device_map=DEV, torch_dtype=dtype, **cfg)
        sd = R.make_state_dict(m)
        m.load_state_dict(sd, strict=True)
        m.sample = False
        _MODELS.clear()
        _MODELS[key] = (m, sd)
    return _MODELS[key]


@pytest.mark.gpu
def test_decode_shipped_width_t2i2v_image(flux_ae):
    """the default t2i2v image: latent 16 x 72 x 128 -> 576 x 1024"""
    m, sd = _model(flux_ae, R.SHIPPED)
    z = torch.randn(1, 16, 1, 72, 128, generator=_gen(1), device=DEV).to(BF)
    with torch.inference_mode():
        ours = m.decode(z)
        torch.cuda.synchronize()
        sd32 = {k: v.to(DEV) for k, v in sd.items()}
        truth = R.decode(sd32, R.SHIPPED, z.float())
        ref = R.decode({k: v.to(BF) for k, v in sd32.items()}, R.SHIPPED, z)
    assert ours.shape == (1, 3, 1, 576, 1024) and ours.dtype == BF
    assert_parity(ours, truth, ref, "Flux AE decode 16x72x128 -> 576x1024 (shipped widths)")


@pytest.mark.gpu
def test_encode_shipped_width_256px(flux_ae):
    m, sd = _model(flux_ae, R.SHIPPED)
    x = (0.5 * torch.randn(1, 3, 1, 256, 256, generator=_gen(2), device=DEV)).to(BF)
    with torch.inference_mode():
        ours = m.encode(x)
        torch.cuda.synchronize()
        sd32 = {k: v.to(DEV) for k, v in sd.items()}
        truth = R.encode_mode(sd32, R.SHIPPED, x.float())
        ref = R.encode_mode({k: v.to(BF) for k, v in sd32.items()}, R.SHIPPED, x)
    assert ours.shape == (1, 16, 1, 32, 32)
    assert_parity(ours, truth, ref, "Flux AE encode 256x256 (shipped widths)")


@pytest.mark.gpu
def test_small_geometry_vs_reference_golden(flux_ae):
    g = np.load(GOLDEN)
    m, sd = _model(flux_ae, R.SMALL)
    z, x = torch.from_numpy(g["z"]).to(DEV), torch.from_numpy(g["x"]).to(DEV)
    sdb = {k: v.to(DEV, BF) for k, v in sd.items()}
    with torch.inference_mode():
        dec, enc = m.decode(z.to(BF)), m.encode(x.to(BF))
        dec_r, enc_r = R.decode(sdb, R.SMALL, z.to(BF)), R.encode_mode(sdb, R.SMALL, x.to(BF))
    assert_parity(dec, torch.from_numpy(g["dec"]), dec_r, "Flux AE small decode vs reference golden")
    assert_parity(enc, torch.from_numpy(g["enc"]), enc_r, "Flux AE small encode vs reference golden")


# ---------------------------------------------------------------------------------------------------------------- distilled
_DCFG = dict(configs.GOLDEN["hd64_liger_split"][0], cond_embed=False)   # guidance_embed=True, no cond_embed: flux-dev's flags
_DSHAPE = (1, 1, 4, 6, 24)   # B, T, h, w (patches), L_txt


def _denoise_inputs(dtype, device):
    B, T, h, w, L = _DSHAPE
    inp = torch_inputs(_DCFG, B, T, h, w, L, dtype=dtype, device=device)
    inp.pop("timesteps"), inp.pop("guidance")
    return inp


def _oracle_loop(sd, inp, timesteps, guidance):
    fn = SO.mmdit_fn(sd, _DCFG)
    img = inp["img"]
    kw = {k: v for k, v in inp.items() if k != "img"}
    g_vec = torch.full((img.shape[0],), guidance, dtype=img.dtype)
    for tc, tp in zip(timesteps[:-1], timesteps[1:]):
        pred = fn(img=img, timesteps=torch.full((img.shape[0],), tc, dtype=img.dtype), guidance=g_vec, **kw)
        img = img + (tp - tc) * pred
    return img


def _flux(dtype=BF):
    from open_sora_amd import mmdit

    m = mmdit.Flux(device_map=DEV, torch_dtype=dtype, **_DCFG)
    m.load_state_dict(torch_params(_DCFG, dtype=dtype, device=DEV), strict=True)
    return m


@pytest.mark.gpu
def test_distilled_denoiser_three_steps(flux_ae):
    from open_sora_amd import sampling

    ts = sampling.get_schedule(3, 24, 1)
    model = _flux()
    with torch.inference_mode():
        inp = _denoise_inputs(BF, DEV)
        ours = sampling.DistilledDenoiser().denoise(model, **dict(inp, timesteps=ts, guidance=4.0))
        graphed = sampling.DistilledDenoiser().denoise(model, **dict(inp, timesteps=ts, guidance=4.0, hip_graph=True))
        torch.cuda.synchronize()
        truth = _oracle_loop(torch_params(_DCFG), _denoise_inputs(torch.float32, "cpu"), ts, 4.0)
        ref = _oracle_loop(torch_params(_DCFG, dtype=BF), _denoise_inputs(BF, "cpu"), ts, 4.0)
    assert_parity(ours, truth, ref, "DistilledDenoiser, 3 steps, tiny flux-style model")
    assert torch.equal(graphed, ours), "hipGraph replay differs from the eager loop"


@pytest.mark.gpu
def test_image_stage_end_to_end(flux_ae, hip_lib):
    """noise -> DistilledDenoiser -> unpack -> AutoEncoder.decode on the GPU against the same composition on the CPU emulation"""
    from open_sora_amd import mmdit, sampling

    B, T, h, w, L = _DSHAPE
    ts = sampling.get_schedule(3, h * w, 1)

    def stage(device, ae, model):
        inp = _denoise_inputs(BF, device)
        x = sampling.DistilledDenoiser().denoise(model, **dict(inp, timesteps=ts, guidance=4.0))
        lat = SO.unpack(x, h, w, T)                        # [1, 16, 1, 8, 12] -> 32 x 48 pixels (4x AE)
        return ae.decode(lat)

    with torch.inference_mode():
        ae, _ = _model(flux_ae, R.SMALL)
        gpu = stage(DEV, ae, _flux()).float().cpu()
        mmdit.set_ops_for_testing(cpu_ops_flux)
        try:
            ae_c = flux_ae.AutoEncoderFlux(from_pretrained=None, device_map="cpu", torch_dtype=BF, **R.SMALL)
            ae_c.load_state_dict(R.make_state_dict(ae_c), strict=True)
            from open_sora_amd import mmdit as M
            fc = M.Flux(device_map="cpu", torch_dtype=BF, **_DCFG)
            fc.load_state_dict(torch_params(_DCFG, dtype=BF), strict=True)
            cpu = stage("cpu", ae_c, fc).float()
        finally:
            mmdit.set_ops_for_testing(hip_lib)
    assert gpu.shape == (1, 3, 1, 32, 48) and torch.isfinite(gpu).all()
    scale = max(1.0, float(cpu.abs().max()))
    d = float((gpu - cpu).abs().max())
    print(f"image stage GPU vs CPU composition: max-abs {d:.3e} (scale {scale:.3e})")
    assert d <= 3e-2 * scale
