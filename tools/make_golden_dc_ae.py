"""Record tests/golden/dc_ae_small.npz: the REFERENCE's own Video DC-AE decoder (opensora/models/dc_ae/models/dc_ae.py, imported
unmodified through oracle.ref_loader on the CPU, fp32) on the small test geometry with the seeded weights of
tests/dc_ae_restatement.py.  The fixture holds arrays and the list of the reference's `decoder.*` state-dict key names only; the
weights are regenerated from the seed.

    python tools/make_golden_dc_ae.py

Three decodes: untiled [1, 32, 2, 2, 2] -> [1, 3, 8, 64, 64]; a single frame [1, 32, 1, 2, 2] -> [1, 3, 1, 64, 64] (the T == 1
branch of the upsample blocks); tiled in T, H and W (spatial_tile_size 128, temporal_tile_size 16) [1, 32, 6, 6, 5] ->
[1, 3, 24, 192, 160] with a short last tile on every axis.  The tiled output is 8.8 MB, so a fixed index subset is kept: the frames
TILED_T at the rows TILED_ROWS (all columns) and at the columns TILED_COLS (all rows).  The seams lie at frame 12 (cross-fade over
frames 12 .. 15), row 96 and column 96 (cross-fades over 96 .. 127): the subset holds the first, a middle and the last slice of
every cross-fade and both neighbours outside it.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from tests import dc_ae_restatement as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "dc_ae_small.npz")

TILED = dict(spatial_tile_size=128, temporal_tile_size=16, tile_overlap_factor=0.25)
TILED_T = [0, 11, 12, 13, 14, 15, 16, 23]
TILED_ROWS = [0, 95, 96, 97, 111, 126, 127, 128, 191]
TILED_COLS = [0, 95, 96, 97, 111, 126, 127, 128, 159]


def inputs():
    """the three latents, seeded, bf16-representable"""
    g = torch.Generator().manual_seed(11)
    return tuple(torch.randn(s, generator=g).bfloat16().float() for s in ((1, 32, 2, 2, 2), (1, 32, 1, 2, 2), (1, 32, 6, 6, 5)))


def tiled_subset(dec: torch.Tensor):
    d = dec[:, :, TILED_T]
    return d[:, :, :, TILED_ROWS, :].contiguous(), d[:, :, :, :, TILED_COLS].contiguous()


def reference_module():
    """the reference's dc_ae.py, unmodified: parent packages by path and a stand-in for the absent omegaconf (only its names
    are touched at import time)"""
    ref_loader.install()
    r = os.path.join(ref_loader.REF_ROOT, "opensora", "models", "dc_ae")
    if "opensora.models.dc_ae" not in sys.modules:
        ref_loader._pkg("opensora.models.dc_ae", r)
        ref_loader._pkg("opensora.models.dc_ae.models", os.path.join(r, "models"))
        ref_loader._pkg("opensora.models.dc_ae.models.nn", os.path.join(r, "models", "nn"))
    if "omegaconf" not in sys.modules:
        m = types.ModuleType("omegaconf")
        m.MISSING = "???"
        m.OmegaConf = type("OmegaConf", (), {})
        sys.modules["omegaconf"] = m
    import importlib

    return importlib.import_module("opensora.models.dc_ae.models.dc_ae")


def reference_dcae(cfg: dict, **tiling):
    """the reference's DCAE for a restatement geometry, decoder loaded with the seeded weights (its encoder keeps its own init)"""
    D = reference_module()
    kw = dict(width_list=tuple(cfg["width_list"]), block_type=list(cfg["block_type"]), norm="rms3d", is_video=True)
    enc = D.EncoderConfig(in_channels=cfg["in_channels"], latent_channels=cfg["latent_channels"], depth_list=tuple(cfg["depth_list"]),
                          downsample_block_type="Conv", temporal_downsample=tuple(cfg["temporal_upsample"]), **kw)
    dec = D.DecoderConfig(in_channels=cfg["in_channels"], latent_channels=cfg["latent_channels"], depth_list=tuple(cfg["depth_list"]),
                          upsample_block_type="InterpolateConv", act="silu", out_norm="rms3d",
                          temporal_upsample=tuple(cfg["temporal_upsample"]), **kw)
    c = D.DCAEConfig(in_channels=cfg["in_channels"], latent_channels=cfg["latent_channels"], time_compression_ratio=4,
                     spatial_compression_ratio=32, encoder=enc, decoder=dec, **tiling)
    m = D.DCAE(c)
    m.decoder.disc_off_grad_ckpt = True
    keys = [k for k in m.state_dict() if k.startswith("decoder.")]
    missing, unexpected = m.load_state_dict(R.make_state_dict(R.param_shapes(cfg)), strict=False)
    assert not unexpected and all(k.startswith("encoder.") for k in missing), (missing, unexpected)
    return m.eval(), keys


def main():
    if not ref_loader.available():
        raise SystemExit(f"needs the reference tree at {ref_loader.REF_ROOT}")
    za, zb, zc = inputs()
    with torch.no_grad():
        ref, keys = reference_dcae(R.SMALL)
        dec_a, dec_b = ref.decode(za), ref.decode(zb)
        tiled, _ = reference_dcae(R.SMALL, use_spatial_tiling=True, use_temporal_tiling=True, **TILED)
        dec_c = tiled.decode(zc)
    assert tuple(dec_c.shape) == (1, 3, 24, 192, 160), dec_c.shape
    by_rows, by_cols = tiled_subset(dec_c)
    np.savez_compressed(OUT, keys=np.array(keys), z_a=za.numpy(), dec_a=dec_a.numpy(), z_b=zb.numpy(), dec_b=dec_b.numpy(),
                        z_c=zc.numpy(), dec_c_rows=by_rows.numpy(), dec_c_cols=by_cols.numpy(),
                        tiled_t=np.array(TILED_T), tiled_rows=np.array(TILED_ROWS), tiled_cols=np.array(TILED_COLS))
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): dec_a {tuple(dec_a.shape)} |max| {float(dec_a.abs().max()):.3f}, "
          f"dec_b {tuple(dec_b.shape)}, dec_c {tuple(dec_c.shape)}")


if __name__ == "__main__":
    main()
