"""Record tests/golden/t5_small.npz: the output of the installed `transformers` T5EncoderModel (random T5Config, no download; CPU)
on the small test geometry with the seeded weights of tests/t5_restatement.py.  The fixture holds arrays and the list of the
model's state-dict key names only; the weights are regenerated from the seed by `small_state_dict()`.

    python tools/make_golden_t5.py

Recorded: `input_ids` [2, 192] (distances pass relative_attention_max_distance = 128), `last_hidden_state` of the fp32 model, the
bf16 model's `last_hidden_state` (as bf16 bit patterns), and `compute_bias(L, L)` of block 0 for L = 192 and 520 -- checked to depend
on j - i alone and stored as the [H, 2 L - 1] table of distances (the [H, L, L] matrix of L = 520 would be 4 MB).
"""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import t5_restatement as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "t5_small.npz")
B, L = 2, 192
BIAS_LENGTHS = (192, 520)


def small_state_dict() -> dict:
    return R.make_state_dict(R.SMALL)


def input_ids() -> torch.Tensor:
    return torch.randint(0, R.SMALL["vocab_size"], (B, L), generator=torch.Generator().manual_seed(31))


@contextlib.contextmanager
def _without_specless_modules():
    """transformers probes optional packages with importlib.util.find_spec, which raises on a sys.modules entry that has no
    __spec__ -- the stand-in packages oracle.ref_loader installs (flash_attn, ...) when an earlier test of the same process loaded the
    reference.  Hide such entries while transformers imports, builds or runs a model."""
    def specless(n):
        m = sys.modules.get(n)
        return m is not None and n != "__main__" and getattr(m, "__spec__", None) is None

    hidden = {n: m for n, m in sys.modules.items() if specless(n.partition(".")[0])}      # whole stand-in packages only
    for n in hidden:
        del sys.modules[n]
    try:
        yield
    finally:
        for n, m in hidden.items():
            sys.modules.setdefault(n, m)


def hf_model(cfg: dict, sd: dict, dtype=torch.float32):
    """transformers' T5EncoderModel of this geometry, loaded strictly with `sd`"""
    with _without_specless_modules():
        return _hf_model(cfg, sd, dtype)


def hf_last_hidden_state(m, ids: torch.Tensor) -> torch.Tensor:
    """the call of conditioner.py:48-53"""
    with _without_specless_modules(), torch.no_grad():
        return m(input_ids=ids, attention_mask=None, output_hidden_states=False)["last_hidden_state"]


def _hf_model(cfg: dict, sd: dict, dtype):
    from transformers import T5Config, T5EncoderModel

    c = T5Config(vocab_size=cfg["vocab_size"], d_model=cfg["d_model"], d_kv=cfg["d_kv"], d_ff=cfg["d_ff"], num_layers=cfg["num_layers"],
                 num_heads=cfg["num_heads"], relative_attention_num_buckets=cfg["relative_attention_num_buckets"],
                 relative_attention_max_distance=cfg["relative_attention_max_distance"], layer_norm_epsilon=cfg["layer_norm_epsilon"],
                 feed_forward_proj="gated-gelu", dropout_rate=0.0, is_encoder_decoder=False, use_cache=False)
    m = T5EncoderModel(c)
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    return m.to(dtype).eval()


def hf_bias_table(m, n: int) -> torch.Tensor:
    att = m.encoder.block[0].layer[0].SelfAttention
    with _without_specless_modules(), torch.no_grad():
        full = att.compute_bias(n, n)
    assert tuple(full.shape) == (1, att.n_heads, n, n), full.shape
    return R.toeplitz_table(full[0].float())


def main():
    sd = small_state_dict()
    ids = input_ids()
    m = hf_model(R.SMALL, sd)
    keys = list(m.state_dict())
    assert keys == list(R.param_shapes(R.SMALL)), "tests/t5_restatement.param_shapes no longer lists transformers' keys"
    with torch.no_grad():
        out32 = hf_last_hidden_state(m, ids)
        tables = {f"bias_{n}": hf_bias_table(m, n).numpy() for n in BIAS_LENGTHS}
        out16 = hf_last_hidden_state(hf_model(R.SMALL, sd, torch.bfloat16), ids)
    assert out16.dtype == torch.bfloat16 and tuple(out32.shape) == (B, L, R.SMALL["d_model"])
    np.savez_compressed(OUT, keys=np.array(keys), input_ids=ids.numpy(), last_hidden_state=out32.numpy(),
                        last_hidden_state_bf16_bits=out16.view(torch.int16).numpy(), **tables)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): last_hidden_state {tuple(out32.shape)} |max| {float(out32.abs().max()):.3f}, "
          f"bf16 run relL2 {float((out16.float() - out32).norm() / out32.norm()):.3e}")


if __name__ == "__main__":
    main()
