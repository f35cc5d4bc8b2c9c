"""Time the LoRA merge (osk_lora_merge_bf16) at every block-weight shape of the XL and the 11B denoiser, r = 16 and r = 64, on the
GPU with device events after a warm-up, beside the same arithmetic done by torch in f32 on the same card:

  merge_us        one osk_lora_merge_bf16 launch, one adapter: reads W, writes W' (A and B stay in cache)
  hbm_fraction    (2 N K 2 bytes / 8.0 TB/s) / merge time: the share of the HBM roofline (the kernel is bound by bandwidth, not by its
                  2 N K r FLOPs: 0.03 - 0.13 of the bf16 MFMA time at these ranks)
  torch_f32_us    (W.float() + s * (B.float() @ A.float())).bfloat16(): the fallback of mmdit._lora_merge, for comparison

A plan build merges each weight once, cold.  To keep the timed launches out of the 256 MB last-level cache every launch works on
another (W, W') pair of a pool of at least --pool-mib MiB that is walked round-robin; a window is --iters launches after one pass
over the pool as warm-up.  The per-geometry total is what load_lora adds to the next plan build for an adapter on every Linear of
every block.

    python tools/lora_time.py [--iters 2000] [--pool-mib 1024] [--out profiles/lora_time.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF = torch.bfloat16
HBM_PEAK = 8.0e12     # bytes / s, MI355X HBM3E specification


def block_shapes(cfg: dict) -> list:
    """(name, N, K, how many per model) of every nn.Linear inside the double / single blocks"""
    D, nd, ns = cfg["hidden_size"], cfg["depth"], cfg["depth_single_blocks"]
    R = int(D * cfg["mlp_ratio"])
    out = [("double.attn.proj", D, D, 2 * nd), ("double.mlp.0", R, D, 2 * nd), ("double.mlp.2", D, R, 2 * nd), ("double.mod.lin", 6 * D, D, 2 * nd),
           ("single.linear2", D, D + R, ns), ("single.modulation.lin", 3 * D, D, ns)]
    if cfg["fused_qkv"]:
        out += [("double.attn.qkv", 3 * D, D, 2 * nd), ("single.linear1", 3 * D + R, D, ns)]
    else:
        out += [("double.attn.q|k|v_proj", D, D, 6 * nd), ("single.q|k_proj", D, D, 2 * ns), ("single.v_mlp", D + R, D, ns)]
    return out


def timed(fn, n_pool: int, iters: int) -> float:
    for i in range(n_pool):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i % n_pool)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--pool-mib", type=int, default=1024)
    ap.add_argument("--models", default="XL,11B")
    ap.add_argument("--ranks", default="16,64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from open_sora_amd import _C
    from open_sora_amd.configs import MMDIT

    if not torch.cuda.is_available():
        raise SystemExit("lora_time.py measures on the GPU: no device found")
    torch.cuda.set_device(0)
    dev = "cuda:0"

    def emit(row):
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out), "a") as f:
                f.write(json.dumps(row) + "\n")

    g = torch.Generator(device=dev).manual_seed(1)
    for model in a.models.split(","):
        cfg = MMDIT[model]
        for r in (int(x) for x in a.ranks.split(",")):
            tot_merge = tot_torch = tot_bytes = 0.0
            for name, N, K, count in block_shapes(cfg):
                nbytes = 2.0 * N * K * 2
                n_pool = max(2, -(-a.pool_mib * 2 ** 20 // int(nbytes)))
                ws = [(torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(BF) for _ in range(n_pool)]
                outs = [torch.empty(N, K, dtype=BF, device=dev) for _ in range(n_pool)]
                A = (torch.randn(r, K, device=dev, generator=g) * K ** -0.5).to(BF)
                B = (torch.randn(N, r, device=dev, generator=g) * 0.1).to(BF)
                ads = [(A, B, 2.0)]
                iters = max(20, min(a.iters, int(a.iters * 21.2e6 / nbytes)))      # the same bytes per window at every shape, at least 20 launches
                ms = timed(lambda i: _C.lora_merge(ws[i], outs[i], ads), n_pool, iters)

                def torch_merge(i):
                    outs[i].copy_((ws[i].float() + 2.0 * (B.float() @ A.float())).to(BF))

                ms_t = timed(torch_merge, n_pool, max(10, iters // 8))
                emit(dict(what="lora_merge", model=model, linear=name, N=N, K=K, r=r, per_model=count, pool=n_pool, launches=iters,
                          merge_us=round(1e3 * ms, 2), hbm_fraction=round(nbytes / HBM_PEAK / (ms * 1e-3), 3),
                          tb_per_s=round(nbytes / (ms * 1e-3) / 1e12, 3), torch_f32_us=round(1e3 * ms_t, 2),
                          torch_over_merge=round(ms_t / ms, 2)))
                tot_merge += count * ms
                tot_torch += count * ms_t
                tot_bytes += count * nbytes
                del ws, outs
                torch.cuda.empty_cache()
            emit(dict(what="lora_merge_all_block_weights", model=model, r=r, merge_ms=round(tot_merge, 3),
                      hbm_fraction=round(tot_bytes / HBM_PEAK / (tot_merge * 1e-3), 3), torch_f32_ms=round(tot_torch, 3)))


if __name__ == "__main__":
    main()
