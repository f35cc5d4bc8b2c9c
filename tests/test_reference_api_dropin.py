"""The drop-in at the API level: the REFERENCE'S OWN `prepare_api` / `api_fn`
(opensora/utils/sampling.py:562-726, executed from the reference tree through oracle.ref_loader.extract_defs -- its module
cannot be imported: mmengine / peft / colossalai are absent) drives THIS package's modules unchanged: `MMDiTModel` as
`model`, a VAE with the reference's `encode / decode / compression` interface as `model_ae`.  The package ships no copy of
that host glue (round 2's open_sora_amd/api.py was one and is gone): switching = passing these modules to the reference's
own function.  Checked on the CPU emulation of the kernels: the reference pipeline ran end to end on our modules
(oracle/make_golden_refchecks.py records its result in tests/golden/ref_checks.npz; the case is tests/ref_cases.py), and that result equals the same
pipeline composed from this package's sampler pieces (open_sora_amd.sampling) to one bf16 rounding per Euler step (the
reference updates x in bf16 torch ops, ours in one f32 kernel).  CPU only."""
import numpy as np
import pytest
import torch

from tests import cpu_ops
from tests.ref_cases import BF, COND_TYPES, GOLDEN, ClipStub, T5Stub, api_case


@pytest.mark.parametrize("cond_type", COND_TYPES)
def test_reference_prepare_api_drives_our_modules(hip_lib, cond_type):
    from open_sora_amd import mmdit, sampling

    mmdit.set_ops_for_testing(cpu_ops)
    try:
        model, ae, kw, pixels, _ = api_case(cond_type)
        height, width, frames, steps, seed = (kw[k] for k in ("height", "width", "num_frames", "num_steps", "seed"))
        theirs = torch.from_numpy(np.load(GOLDEN)[f"api_{cond_type}"])

        # ---- the same pipeline composed from this package's pieces
        T_lat = (frames - 1) // 4 + 1
        with torch.inference_mode():
            z = sampling.get_noise(1, height, width, T_lat, torch.device("cpu"), BF, seed, patch_size=2, channel=16)
            Hl, Wl = z.shape[-2:]
            n_img = T_lat * (Hl // 2) * (Wl // 2)
            text3 = ["a cat", "", ""]
            txt, y_vec = T5Stub()(text3, added_tokens=n_img).to(BF), ClipStub()(text3).to(BF)
            img_ids, txt_ids = sampling.prepare_ids(3, T_lat, Hl, Wl, txt.shape[1], "cpu", BF)
            masks, masked_ref = torch.zeros(1, 1, T_lat, Hl, Wl, dtype=BF), torch.zeros(1, 16, T_lat, Hl, Wl, dtype=BF)
            lat_ref = None
            if cond_type == "i2v_head":
                lat_ref = ae.encode(pixels[None].to(BF))
                masks[:, :, 0] = 1
                masked_ref[:, :, 0] = lat_ref[:, :, 0]
            x = sampling.I2VDenoiser().denoise(
                model, img=sampling.pack(z).repeat(3, 1, 1), timesteps=sampling.get_schedule(steps, (Hl // 2) * (Wl // 2), T_lat),
                guidance=7.5, guidance_img=3.0, masks=masks, masked_ref=masked_ref, text_osci=True, image_osci=True,
                scale_temporal_osci="i2v" in cond_type, img_ids=img_ids, txt=txt, txt_ids=txt_ids, y_vec=y_vec)
            x = sampling.unpack(x, height, width, T_lat)
            if cond_type == "i2v_head":
                x[0, :, :1] = lat_ref[0, :, :1]
            ours = ae.decode(x)[:, :, :frames]
        assert ours.shape == theirs.shape and torch.isfinite(theirs.float()).all()
        scale = max(1.0, theirs.float().abs().max().item())
        assert (ours.float() - theirs.float()).abs().max().item() <= 3e-2 * scale
    finally:
        mmdit.set_ops_for_testing(hip_lib)
