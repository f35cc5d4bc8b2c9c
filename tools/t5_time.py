"""Time the T5 text encoder (open_sora_amd.t5) at the geometry of T5-v1.1-XXL with random bf16 weights, B = 2 prompts ([text; neg]) of
L = 512 tokens, on the GPU with device events after a warm-up:

  forward     T5Encoder.forward, all layers;
  attention   osk_attention_relbias_bf16 alone at [2, 512, 64 heads x 64], q / k / v in place in a fused projection buffer, two
              ways: `warm` = back-to-back launches on ONE buffer (after the first launch the operands sit in L2 / Infinity
              Cache -- as they do in the model, where the projection GEMM has just written them), `rotating` = the launches walk
              over ROT buffers whose total exceeds the 256 MB Infinity Cache, so every launch reads its operands from HBM;
  torch       for comparison, the plain-PyTorch encoder of the same weights (tests/t5_restatement.py: matmul, softmax) in bf16 on
              the same GPU in the same process, and its attention alone (--no-torch skips both).

FLOPs are counted algorithmically: per layer 2 * B * L * d_model * (4 * H * 64 + 3 * d_ff) in the Linears and 4 * B * H * L^2 * 64 in
the attention; fractions are of the 2.5 PFLOP/s bf16 peak.

Defaults give windows of about a second (50 forwards, 2000 kernel launches), after 5 warm-up calls.  The kernel figures are means
over such a window, not per-launch profiler times.

    python tools/t5_time.py [--layers 24] [--iters 50] [--no-torch] [--out profiles/t5_time.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import t5_restatement as R  # noqa: E402

PEAK = 2.5e15
BF = torch.bfloat16
ROT = 16                    # fused q|k|v buffers of the rotating measurement: 16 x 25 MB at the default shape


def timed(fn, iters: int, warmup: int = 5) -> float:
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
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from open_sora_amd import _C, t5

    dev = "cuda:0"
    torch.cuda.set_device(0)
    cfg = dict(R.XXL_LAYER, vocab_size=32128, num_layers=a.layers)
    B, L, H, hd, D, Fd = a.batch, a.tokens, cfg["num_heads"], cfg["d_kv"], cfg["d_model"], cfg["d_ff"]
    sd = {k: v.to(BF) for k, v in R.make_state_dict(cfg, seed=1, device=dev).items()}
    with torch.device(dev):
        m = t5.T5Encoder(t5.T5EncoderConfig(**cfg)).to(BF)
    m.load_state_dict(sd)
    ids = torch.randint(0, cfg["vocab_size"], (B, L), device=dev)
    lin_flops = a.layers * 2.0 * B * L * D * (4 * H * hd + 3 * Fd)
    att_flops = a.layers * 4.0 * B * H * L * L * hd

    def emit(row):
        print(json.dumps(row), flush=True)
        if a.out:
            with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "a") as f:
                f.write(json.dumps(row) + "\n")

    qkv = torch.randn(B, L, 3 * H * hd, device=dev).to(BF)
    q, k, v = qkv[:, :, : H * hd], qkv[:, :, H * hd: 2 * H * hd], qkv[:, :, 2 * H * hd:]
    table = m._plan().table(m.cfg, L)
    out = torch.empty(B, L, H * hd, dtype=BF, device=dev)
    with torch.inference_mode():
        ms = timed(lambda: m(ids), a.iters)
        emit(dict(what="t5_forward_hip", layers=a.layers, B=B, L=L, ms=round(ms, 3), linear_gflop=round(lin_flops / 1e9, 1),
                  attention_gflop=round(att_flops / 1e9, 1), frac_peak=round((lin_flops + att_flops) / (ms * 1e-3) / PEAK, 4)))
        n_k = 40 * a.iters
        ms_k = timed(lambda: _C.attention_relbias(q, k, v, out, H, hd, 1.0, table), n_k)
        bufs = [torch.randn(B, L, 3 * H * hd, device=dev).to(BF) for _ in range(ROT)]
        views = [(t[:, :, : H * hd], t[:, :, H * hd: 2 * H * hd], t[:, :, 2 * H * hd:]) for t in bufs]
        turn = [0]

        def rotating():
            qr, kr, vr = views[turn[0] % ROT]
            turn[0] += 1
            _C.attention_relbias(qr, kr, vr, out, H, hd, 1.0, table)

        ms_r = timed(rotating, n_k, warmup=ROT)
        emit(dict(what="attention_relbias_hip", B=B, L=L, H=H, launches=n_k, ms_warm=round(ms_k, 4), ms_rotating=round(ms_r, 4),
                  frac_peak_warm=round(att_flops / a.layers / (ms_k * 1e-3) / PEAK, 4),
                  frac_peak_rotating=round(att_flops / a.layers / (ms_r * 1e-3) / PEAK, 4),
                  share_of_forward_warm=round(a.layers * ms_k / ms, 4)))
        if not a.no_torch:
            ms_t = timed(lambda: R.encode(sd, cfg, ids), a.iters)
            emit(dict(what="t5_forward_torch_bf16", layers=a.layers, B=B, L=L, ms=round(ms_t, 3), hip_over_torch=round(ms / ms_t, 3)))
            bias = R.compute_bias(sd, cfg, L)
            q4, k4, v4 = (t.reshape(B, L, H, hd) for t in (q, k, v))
            ms_ta = timed(lambda: R.attention(q4, k4, v4, bias), 4 * a.iters)
            emit(dict(what="attention_torch_bf16", B=B, L=L, H=H, launches=4 * a.iters, ms_warm=round(ms_ta, 4), hip_over_torch=round(ms_k / ms_ta, 3)))


if __name__ == "__main__":
    main()
