"""Record tests/golden/clip_small.npz: the output of the installed `transformers` CLIPTextModel (random CLIPTextConfig, no download;
CPU) on the small test geometry with the seeded weights of tests/clip_restatement.py.  The fixture holds arrays and the list of the
model's state-dict key names only; the weights are regenerated from the seed by `small_state_dict()`.

    python tools/make_golden_clip.py

Recorded: `input_ids` [3, 77] (the largest id of the three rows at positions 5, 40 and 76: the rows transformers pools),
`last_hidden_state` and `pooler_output` of the fp32 model, and the bf16 model's two outputs as bf16 bit patterns.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import clip_restatement as R  # noqa: E402
from tools.make_golden_t5 import _without_specless_modules  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "clip_small.npz")
B, L = 3, 77
EOS_AT = (5, 40, 76)


def small_state_dict() -> dict:
    return R.make_state_dict(R.SMALL)


def input_ids() -> torch.Tensor:
    """ids below the largest one, which stands once per row (CLIP's end-of-text token is the highest id of its vocabulary)"""
    top = R.SMALL["vocab_size"] - 1
    ids = torch.randint(0, top, (B, L), generator=torch.Generator().manual_seed(37))
    for b, at in enumerate(EOS_AT):
        ids[b, at] = top
    return ids


def hf_model(cfg: dict, sd: dict, dtype=torch.float32, **overrides):
    """transformers' CLIPTextModel of this geometry, loaded strictly with `sd`"""
    with _without_specless_modules():
        from transformers import CLIPTextConfig, CLIPTextModel

        kw = dict(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                  num_hidden_layers=cfg["num_hidden_layers"], num_attention_heads=cfg["num_attention_heads"],
                  max_position_embeddings=cfg["max_position_embeddings"], layer_norm_eps=cfg["layer_norm_eps"],
                  eos_token_id=cfg["eos_token_id"], bos_token_id=0, pad_token_id=1, hidden_act="quick_gelu", attention_dropout=0.0)
        kw.update(overrides)
        m = CLIPTextModel(CLIPTextConfig(**kw))
        if sd is not None:
            m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
        return m.to(dtype).eval()


def hf_outputs(m, ids: torch.Tensor):
    """the call of conditioner.py:48-53 -> (last_hidden_state, pooler_output)"""
    with _without_specless_modules(), torch.no_grad():
        out = m(input_ids=ids, attention_mask=None, output_hidden_states=False)
    return out["last_hidden_state"], out["pooler_output"]


def main():
    sd = small_state_dict()
    ids = input_ids()
    m = hf_model(R.SMALL, sd)
    keys = list(m.state_dict())
    assert keys == list(R.param_shapes(R.SMALL)), "tests/clip_restatement.param_shapes no longer lists transformers' keys"
    h32, p32 = hf_outputs(m, ids)
    h16, p16 = hf_outputs(hf_model(R.SMALL, sd, torch.bfloat16), ids)
    assert h16.dtype == p16.dtype == torch.bfloat16 and tuple(h32.shape) == (B, L, R.SMALL["hidden_size"]) and tuple(p32.shape) == (B, R.SMALL["hidden_size"])
    assert all(torch.equal(p32[b], h32[b, at]) for b, at in enumerate(EOS_AT)), "transformers pooled another row"
    np.savez_compressed(OUT, keys=np.array(keys), input_ids=ids.numpy(), last_hidden_state=h32.numpy(), pooler_output=p32.numpy(),
                        last_hidden_state_bf16_bits=h16.view(torch.int16).numpy(), pooler_output_bf16_bits=p16.view(torch.int16).numpy())
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): last_hidden_state {tuple(h32.shape)} |max| {float(h32.abs().max()):.3f}, "
          f"bf16 run relL2 {float((h16.float() - h32).norm() / h32.norm()):.3e}")


if __name__ == "__main__":
    main()
