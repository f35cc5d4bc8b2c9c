"""Record tests/golden/flux_ae_small.npz: the REFERENCE's own Flux 2-D autoencoder (opensora/models/vae/autoencoder_2d.py, imported
through oracle.ref_loader on the CPU, fp32) on the small test geometry with the seeded weights of tests/flux_ae_restatement.py.
The fixture holds arrays only (the latent / image inputs and the reference's outputs); the weights are regenerated from the seed.

    python tools/make_golden_flux_ae.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from tests import flux_ae_restatement as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "flux_ae_small.npz")


def inputs():
    """latent [1, 16, 1, 8, 8] and image [1, 3, 1, 32, 32], seeded, bf16-representable"""
    g = torch.Generator().manual_seed(7)
    z = torch.randn(1, 16, 1, 8, 8, generator=g).bfloat16().float()
    x = (0.5 * torch.randn(1, 3, 1, 32, 32, generator=g)).bfloat16().float()
    return z, x


def reference_ae(cfg: dict):
    ref_loader.install()
    from opensora.models.vae.autoencoder_2d import AutoEncoderFlux

    m = AutoEncoderFlux(from_pretrained=None, device_map="cpu", torch_dtype=torch.float32, **cfg)
    m.load_state_dict(R.make_state_dict(m), strict=True)
    m.sample = False
    return m.eval()


def main():
    if not ref_loader.available():
        raise SystemExit(f"needs the reference tree at {ref_loader.REF_ROOT}")
    ref = reference_ae(R.SMALL)
    z, x = inputs()
    with torch.no_grad():
        dec = ref.decode(z)
        enc = ref.encode(x)
    np.savez_compressed(OUT, z=z.numpy(), x=x.numpy(), dec=dec.numpy(), enc=enc.numpy())
    print(f"wrote {OUT}: dec {tuple(dec.shape)}, enc {tuple(enc.shape)}")


if __name__ == "__main__":
    main()
