"""TEST INFRASTRUCTURE ONLY — record what the reference's own Python returns for the CPU tests that pin the oracle to it.

Run where the reference tree is available (see oracle/ref_loader.py):
    PYTHONDONTWRITEBYTECODE=1 python -m oracle.make_golden_refchecks
It writes tests/golden/ref_checks.npz: recorded results only (arrays and key names), read by
tests/test_oracle_vs_reference.py, tests/test_sampling_oracle.py, tests/test_vae_oracle.py and
tests/test_reference_api_dropin.py, so that those tests run wherever the repository is checked out.  The seeded inputs and
stand-in models come from tests/ref_cases.py, which the tests build them from as well.
"""
from __future__ import annotations

import math
import os
import random
import sys
from dataclasses import dataclass, replace
from enum import Enum

sys.dont_write_bytecode = True

import numpy as np
import torch

from . import configs, synth
from tests.ref_cases import (COND_TYPES, I2V_CASES, MMDIT_NAMES, SCHEDULES, VAE_NAME, ClipStub, T5Stub, api_case, i2v_case,
                             i2v_key, pack_input)

OUT_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ref_checks.npz")


def ref_namespace() -> dict:
    """the reference's sampling / inference / aspect-ratio definitions, executed from its source text (oracle/ref_loader.py)"""
    import einops
    from abc import ABC, abstractmethod
    from torch import Tensor, nn

    from . import ref_loader

    ns = dict(torch=torch, nn=nn, Tensor=Tensor, math=math, os=os, random=random, dataclass=dataclass, replace=replace,
              Enum=Enum, ABC=ABC, abstractmethod=abstractmethod, rearrange=einops.rearrange, repeat=einops.repeat, HFEmbedder=object, MMDiTModel=object)
    ref_loader.extract_defs("opensora/datasets/aspect.py",
                            ["ASPECT_RATIO_LD_LIST", "get_ratio", "get_aspect_ratios_dict", "get_num_pexels_from_name",
                             "get_image_size"], ns)
    ref_loader.extract_defs("opensora/utils/inference.py", ["SamplingMethod", "prepare_inference_condition",
                                                            "collect_references_batch"], ns)
    ref_loader.extract_defs("opensora/utils/sampling.py",
                            ["SamplingOption", "sanitize_sampling_option", "get_oscillation_gs", "Denoiser", "I2VDenoiser",
                             "DistilledDenoiser", "SamplingMethodDict", "time_shift", "get_res_lin_function", "get_schedule",
                             "get_noise", "pack", "unpack", "prepare", "prepare_api"], ns)
    return ns


def _to_f32(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().numpy().copy()   # bf16 values are exact in float32


def main():
    from . import ref_loader

    out = {}
    # ---- the reference MMDiTModel forward, fp32 and bf16, on the synthetic weights and inputs of tests/util.py
    M, _, _ = ref_loader.mmdit()
    for name in MMDIT_NAMES:
        cfg, B, T, h, w, L_txt = configs.GOLDEN[name]
        sd = {k: torch.from_numpy(v) for k, v in synth.make_params(synth.mmdit_param_shapes(cfg), 0).items()}
        inp = {k: torch.from_numpy(v) for k, v in synth.mmdit_inputs(cfg, B, T, h, w, L_txt).items()}
        model = M.Flux(device_map="cpu", torch_dtype=torch.float32, **cfg)
        model.load_state_dict(sd, strict=True)
        inpb = {k: (v if k in ("img_ids", "txt_ids") else v.bfloat16()) for k, v in inp.items()}
        with torch.inference_mode():
            out[f"mmdit_{name}_fp32"] = _to_f32(model(**inp))
            out[f"mmdit_{name}_bf16"] = _to_f32(model.to(torch.bfloat16)(**inpb))
    # ---- sampling.py: get_schedule, pack, unpack, I2VDenoiser.denoise
    ref = ref_namespace()
    for i, (n, L, T, kw) in enumerate(SCHEDULES):
        out[f"schedule_{i}"] = np.array(ref["get_schedule"](n, L, T, **kw), dtype=np.float64)
    z = pack_input()
    out["pack"] = _to_f32(ref["pack"](z))
    out["unpack"] = _to_f32(ref["unpack"](ref["pack"](z), 8 * 16 // 2, 12 * 16 // 2, 3))
    for dtype, osci in I2V_CASES:
        model, z, masks, masked_ref, sched = i2v_case(dtype)
        kw = dict(text_osci=osci, image_osci=osci, scale_temporal_osci=osci)
        want = ref["I2VDenoiser"]().denoise(model, img=ref["pack"](z).repeat(3, 1, 1), timesteps=ref["get_schedule"](*sched),
                                            guidance=7.5, guidance_img=3.0, masks=masks, masked_ref=masked_ref, sigma_min=1e-5, **kw)
        assert want.dtype == dtype
        out[i2v_key(dtype, osci)] = _to_f32(want)
    # ---- the reference's prepare_api / api_fn driving this package's MMDiTModel (on the CPU emulation of the kernels)
    from open_sora_amd import mmdit
    from tests import cpu_ops

    mmdit.set_ops_for_testing(cpu_ops)
    for cond_type in COND_TYPES:
        model, ae, kw, pixels, extra = api_case(cond_type)
        if pixels is not None:
            ref["read_from_path"] = lambda path, image_size, transform_name="resize_crop", p=pixels: p.clone()
        r_opt = ref["sanitize_sampling_option"](ref["SamplingOption"](**kw))
        theirs = ref["prepare_api"](model, ae, T5Stub(), ClipStub(), {})(r_opt, cond_type=cond_type, text=["a cat"], channel=64, **extra)
        out[f"api_{cond_type}"] = _to_f32(theirs)
    # ---- the reference AutoencoderKLCausal3D: state-dict keys, fp32 encode / decode, bf16 encode
    from .make_golden import reference_vae

    cfg, B, T, H, W = configs.VAE_GOLDEN[VAE_NAME]
    vae = reference_vae(cfg)
    out["vae_keys"] = np.array(list(vae.state_dict().keys()))
    x = torch.from_numpy(synth.vae_video(B, T, H, W))
    with torch.inference_mode():
        z_ref = vae.encode(x, sample_posterior=False)
        out["vae_z"] = _to_f32(z_ref)
        out["vae_dec"] = _to_f32(vae.decode(z_ref))
        out["vae_z_bf16"] = _to_f32(vae.to(torch.bfloat16).encode(x.bfloat16(), sample_posterior=False))
    np.savez_compressed(OUT_PATH, **out)
    print(f"wrote {OUT_PATH}: {len(out)} arrays, {os.path.getsize(OUT_PATH)} bytes")


if __name__ == "__main__":
    main()
