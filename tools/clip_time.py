"""Time the CLIP text encoder (open_sora_amd.clip) at the geometry of CLIP ViT-L/14's text tower with random bf16 weights, B = 3
prompts of L = 77 tokens (the denoiser's CFG batch), on the GPU with device events after a warm-up:

  forward        ClipTextModel.forward, all layers: 7 launches per layer + the final LayerNorm, plus the torch embedding and pooling ops;
  transformers   for comparison, the installed transformers' CLIPTextModel with the same weights in bf16 on the same GPU in the same
                 process (--no-transformers skips it);
  kernels        the three new entries alone at the model's shapes, back-to-back on one buffer (warm: the operands sit in L2, as they
                 do in the model, where the previous launch has just written them).

The forward is bound by its launch count, not by FLOPs (1.3 GFLOP per layer at 3 x 77 tokens): the figure to read is the ratio to
transformers and the launches per forward.

Defaults give windows of 200 forwards and 2000 kernel launches, after 10 warm-up calls; the figures are means over such a window.

    python tools/clip_time.py [--layers 12] [--iters 200] [--no-transformers] [--out profiles/clip_time.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import clip_restatement as R  # noqa: E402

BF = torch.bfloat16


def timed(fn, iters: int, warmup: int = 10) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=77)
    ap.add_argument("--no-transformers", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from open_sora_amd import _C, clip

    dev = "cuda:0"
    torch.cuda.set_device(0)
    cfg = dict(R.L_LAYER, vocab_size=49408, num_hidden_layers=a.layers)
    B, L, H, D, Fd = a.batch, a.tokens, cfg["num_attention_heads"], cfg["hidden_size"], cfg["intermediate_size"]
    sd = {k: v.to(BF) for k, v in R.make_state_dict(cfg, seed=1, device=dev).items()}
    with torch.device(dev):
        m = clip.ClipTextModel(clip.ClipTextConfig(**cfg)).to(BF)
    m.load_state_dict(sd)
    ids = torch.randint(0, cfg["vocab_size"] - 1, (B, L), device=dev)
    ids[:, -1] = cfg["vocab_size"] - 1
    flops = a.layers * (2.0 * B * L * D * (4 * D + 2 * Fd) + 2.0 * B * H * L * L * 64)

    def emit(row):
        print(json.dumps(row), flush=True)
        if a.out:
            with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "a") as f:
                f.write(json.dumps(row) + "\n")

    with torch.inference_mode():
        ms = timed(lambda: m(ids), a.iters)
        emit(dict(what="clip_forward_hip", layers=a.layers, B=B, L=L, ms=round(ms, 4), launches=7 * a.layers + 1, gflop=round(flops / 1e9, 2)))
        n_k = 10 * a.iters
        x = torch.randn(B, L, D, device=dev).to(BF)
        w, b = torch.ones(D, device=dev), torch.zeros(D, device=dev)
        qkv = torch.randn(B, L, 3 * D, device=dev).to(BF)
        out = torch.empty(B, L, D, dtype=BF, device=dev)
        ff = torch.empty(1, B * L, Fd, dtype=BF, device=dev)
        fc1, fc1_b = sd["encoder.layers.0.mlp.fc1.weight"], sd["encoder.layers.0.mlp.fc1.bias"].float()
        ms_ln = timed(lambda: _C.layernorm_affine(x, w, b, out, 1e-5), n_k)
        ms_at = timed(lambda: _C.attention_causal(qkv[:, :, :D], qkv[:, :, D: 2 * D], qkv[:, :, 2 * D:], out, H, 64, 0.125), n_k)
        ms_qg = timed(lambda: _C.gemm_quickgelu(x.view(1, B * L, D), fc1, fc1_b, ff), n_k)
        emit(dict(what="clip_kernels_hip", B=B, L=L, launches=n_k, us_layernorm=round(1e3 * ms_ln, 2), us_attention_causal=round(1e3 * ms_at, 2),
                  us_gemm_quickgelu=round(1e3 * ms_qg, 2)))
        if not a.no_transformers:
            from tools.make_golden_clip import hf_model

            with torch.device(dev):
                hf = hf_model(cfg, None, BF)
            hf.load_state_dict(sd, strict=True)
            ms_t = timed(lambda: hf(input_ids=ids, attention_mask=None, output_hidden_states=False), a.iters)
            emit(dict(what="clip_forward_transformers_bf16", layers=a.layers, B=B, L=L, ms=round(ms_t, 4), hip_over_transformers=round(ms / ms_t, 3)))


if __name__ == "__main__":
    main()
