"""The seeded cases of the CPU tests that are pinned to results recorded from the reference's own Python
(tests/golden/ref_checks.npz): the inputs and stand-in models both the tests and the recorder
(oracle/make_golden_refchecks.py) build them from."""
import os

import torch

from oracle import configs
from tests.util import torch_params

BF = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_checks.npz")

MMDIT_NAMES = ("hd64_eager_fused", "hd72_liger_fused", "hd128_liger_split")
# (num_steps, image_seq_len, num_frames, keyword arguments) of the recorded get_schedule calls
SCHEDULES = ((30, 1024, 16, {}), (3, 24, 3, {}), (50, 3600, 33, {}), (7, 100, 5, {"shift": False}),
             (7, 100, 5, {"shift_alpha": 2.5}))
I2V_CASES = [(dt, osci) for osci in (False, True) for dt in (torch.float32, torch.bfloat16)]
VAE_NAME = "c32_lpb1"


def pack_input() -> torch.Tensor:
    return torch.randn(2, 16, 3, 8, 12, generator=torch.Generator().manual_seed(3))


def i2v_case(dtype):
    """the seeded inputs and the stub model of the sampler-loop check: (model, z, masks, masked_ref, schedule arguments).
    The stub's matmul runs in float64 and is rounded once, so its result does not depend on the host's BLAS."""
    torch.manual_seed(0)
    n, T, Hh, Ww = 2, 3, 4, 6
    z = torch.randn(n, 16, T, Hh, Ww).to(dtype)
    masks = torch.zeros(n, 1, T, Hh, Ww, dtype=dtype)
    masks[:, :, 0] = 1
    masked_ref = (torch.randn(n, 16, T, Hh, Ww) * masks.float()).to(dtype)
    W = (torch.randn(64 + 68, 64) * 0.02).double()

    def model(img, cond, timesteps, guidance, **kw):
        return (torch.cat([img.double(), cond.double()], -1) @ W * (1 + timesteps.double()[:, None, None])).to(img.dtype)

    return model, z, masks, masked_ref, (5, (Hh // 2) * (Ww // 2), T)


def i2v_key(dtype, osci) -> str:
    return f"i2v_{'bf16' if dtype == torch.bfloat16 else 'fp32'}_osci{int(osci)}"


COND_TYPES = ("t2v", "i2v_head")


class T5Stub:
    def __call__(self, prompt, added_tokens=0, seq_align=1):
        g = torch.Generator().manual_seed(len(prompt) * 7 + added_tokens % 5)
        return torch.randn(len(prompt), 24, 96, generator=g) * 0.2


class ClipStub:
    def __call__(self, prompt):
        g = torch.Generator().manual_seed(len(prompt) + 3)
        return torch.randn(len(prompt), 48, generator=g)


class AEStub(torch.nn.Module):
    """stand-in VAE with the reference interface (the HIP VAE is tested on the GPU): decode = fixed channel mix, nearest upsample"""
    compression = (4, 8, 8)

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(3, 16, generator=torch.Generator().manual_seed(2)) * 0.1)

    def decode(self, z):
        return torch.einsum("oc,bcthw->bothw", self.w.to(z.dtype), z).repeat_interleave(4, 2)

    def encode(self, x):
        return torch.einsum("oc,bcthw->bothw", self.w.t().to(x.dtype), x)[:, :, ::4][:, :, : (x.shape[2] - 1) // 4 + 1]


def api_case(cond_type):
    """model, stand-in VAE, SamplingOption keywords, the i2v reference pixels (or None) and the extra api_fn keywords of one
    case of tests/test_reference_api_dropin.py"""
    cfg = dict(configs.GOLDEN["hd64_liger_split"][0], guidance_embed=False)
    from open_sora_amd import mmdit

    model = mmdit.Flux(device_map="cpu", torch_dtype=BF, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=BF), strict=True)
    ae = AEStub().to(BF)
    kw = dict(height=64, width=96, num_frames=9, num_steps=3, guidance=7.5, guidance_img=3.0, text_osci=True,
              image_osci=True, scale_temporal_osci=True, seed=5, is_causal_vae=True, temporal_reduction=4, method="i2v")
    extra, pixels = {}, None
    if cond_type == "i2v_head":
        g = torch.Generator().manual_seed(11)
        pixels = torch.randn(3, 5, 64 // 8, 96 // 8, generator=g)   # "pixels" at the stand-in AE's scale
        extra = dict(ref=["some/path.png"])
    return model, ae, kw, pixels, extra
