"""Record tests/golden/dc_ae_enc_small.npz: the REFERENCE's own Video DC-AE encoder (opensora/models/dc_ae/models/dc_ae.py, imported
unmodified through oracle.ref_loader on the CPU, fp32) on the small test geometry with the seeded weights of
tests/dc_ae_enc_restatement.py.  The fixture holds arrays and the list of the reference's state-dict key names only; the weights
are regenerated from the seed.

    python tools/make_golden_dc_ae_enc.py

Four encodes:
  a  [1, 3, 4, 64, 64]  -> [1, 32, 1, 2, 2];
  b  a single frame [1, 3, 1, 64, 32] (the T == 1 branch of both temporal downsamples);
  c  T = 2, [1, 3, 2, 32, 64]: the 3-D shortcut once, the T == 1 branch after it;
  d  tiled in T, H and W (spatial_tile_size 128, temporal_tile_size 16, overlap 0.25: latent tile 4, blend extent 1)
     [1, 3, 20, 160, 128] -> [1, 32, 5, 5, 4], with a short last tile on every axis.
The inputs of a - c are stored.  d's input (1.2 M values) is regenerated from the seed by `input_d()`; the fixture keeps every
SUB-th value of it so that a test can tell a generator that drifted from a wrong encoder.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from tests import dc_ae_enc_restatement as RE  # noqa: E402
from tests import dc_ae_restatement as R  # noqa: E402
from tools.make_golden_dc_ae import reference_module  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "dc_ae_enc_small.npz")
TILED = dict(spatial_tile_size=128, temporal_tile_size=16, tile_overlap_factor=0.25)
SUB = 997
SHAPES = dict(a=(1, 3, 4, 64, 64), b=(1, 3, 1, 64, 32), c=(1, 3, 2, 32, 64), d=(1, 3, 20, 160, 128))


def inputs():
    """the inputs of a - c, seeded, bf16-representable"""
    g = torch.Generator().manual_seed(21)
    return {t: torch.randn(SHAPES[t], generator=g).bfloat16().float() for t in ("a", "b", "c")}


def input_d():
    return torch.randn(SHAPES["d"], generator=torch.Generator().manual_seed(22)).bfloat16().float()


def small_state_dict() -> dict:
    """both halves, encoder first (the reference's order)"""
    sd = dict(R.make_state_dict(RE.enc_param_shapes(RE.SMALL)))
    sd.update(R.make_state_dict(R.param_shapes(R.SMALL)))
    return sd


def reference_dcae_full(enc: dict, dec: dict, **tiling):
    """the reference's DCAE with BOTH halves loaded (strictly) with the seeded weights"""
    D = reference_module()
    kw = dict(norm="rms3d", is_video=True)
    e = D.EncoderConfig(in_channels=enc["in_channels"], latent_channels=enc["latent_channels"], width_list=tuple(enc["width_list"]),
                        depth_list=tuple(enc["depth_list"]), block_type=list(enc["block_type"]), downsample_block_type="Conv",
                        temporal_downsample=tuple(enc["temporal_downsample"]), **kw)
    d = D.DecoderConfig(in_channels=dec["in_channels"], latent_channels=dec["latent_channels"], width_list=tuple(dec["width_list"]),
                        depth_list=tuple(dec["depth_list"]), block_type=list(dec["block_type"]), upsample_block_type="InterpolateConv",
                        act="silu", out_norm="rms3d", temporal_upsample=tuple(dec["temporal_upsample"]), **kw)
    c = D.DCAEConfig(in_channels=enc["in_channels"], latent_channels=enc["latent_channels"], time_compression_ratio=4,
                     spatial_compression_ratio=32, encoder=e, decoder=d, **tiling)
    m = D.DCAE(c)
    m.decoder.disc_off_grad_ckpt = True
    sd = dict(R.make_state_dict(RE.enc_param_shapes(enc)))
    sd.update(R.make_state_dict(R.param_shapes(dec)))
    m.load_state_dict(sd, strict=True)
    return m.eval(), list(m.state_dict())


def main():
    if not ref_loader.available():
        raise SystemExit(f"needs the reference tree at {ref_loader.REF_ROOT}")
    xs = inputs()
    arrays = {}
    with torch.no_grad():
        ref, keys = reference_dcae_full(RE.SMALL, R.SMALL)
        for t, x in xs.items():
            arrays["x_" + t] = x.numpy()
            arrays["z_" + t] = ref.encode(x).numpy()
        tiled, _ = reference_dcae_full(RE.SMALL, R.SMALL, use_spatial_tiling=True, use_temporal_tiling=True, **TILED)
        xd = input_d()
        zd = tiled.encode(xd)
    assert tuple(arrays["z_a"].shape) == (1, 32, 1, 2, 2), arrays["z_a"].shape
    assert tuple(zd.shape) == (1, 32, 5, 5, 4), zd.shape
    np.savez_compressed(OUT, keys=np.array(keys), z_d=zd.numpy(), x_d_sub=xd.flatten()[::SUB].numpy(), **arrays)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): " + ", ".join(f"z_{t} {tuple(arrays['z_' + t].shape)} |max| "
          f"{float(np.abs(arrays['z_' + t]).max()):.3f}" for t in xs) + f", z_d {tuple(zd.shape)} |max| {float(zd.abs().max()):.3f}")


if __name__ == "__main__":
    main()
