"""Time osk_attention_fwd_window_bf16 (frame-window attention: text prefix + one run of image key tiles per 256-row query block)
against full attention, at the kernel level, on two shapes:

  headline   B = 3, H = 16, head_dim 72, 512 text + 16 x 1,024 image tokens (bench.py's step), W in {1, 2, 4, 16}
  long       B = 1, H = 16, head_dim 72, 512 text + 51 x 3,600 image tokens (BASELINE configs[3]),  W in {2, 8}

The baseline arm is the call the model makes without a window: osk_attention_fwd_bounded_bf16 with the tail-split workspace
(_C.attention_fwd).  Both arms get the same q, k, V^T and the same score bound (the FAST body).  Per shape, ONE process: every arm
is warmed up, then the arms alternate, `repeats` rounds of `inner` back-to-back calls each between two device events.  Printed per
arm: the median time, the spread, the visited-tile fraction (text tiles included, mmdit.window_tile_fraction), the time ratio to the
baseline and that ratio over the tile fraction (1.0 = time follows the tiles).  W = 16 at the headline shape has every range full:
it prices the second launch, the merge and the loss of the wide layout and of the tail split.  No threshold is set.

    python tools/attn_window_time.py [--repeats 7] [--out profiles/attn_window_time.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [dict(name="headline", B=3, H=16, hd=72, L_txt=512, N=1024, T=16, windows=(1, 2, 4, 16), inner=8),
          dict(name="long", B=1, H=16, hd=72, L_txt=512, N=3600, T=51, windows=(2, 8), inner=1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="headline,long")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 3, "at least 3 rounds of every arm"

    from open_sora_amd import _C, mmdit

    dev = "cuda:0"
    torch.cuda.set_device(0)

    def emit(row):
        print(json.dumps(row), flush=True)
        if a.out:
            path = a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "a") as f:
                f.write(json.dumps(row) + "\n")

    for s in SHAPES:
        if s["name"] not in a.shapes.split(","):
            continue
        B, H, hd, Lt, N, T = s["B"], s["H"], s["hd"], s["L_txt"], s["N"], s["T"]
        L = Lt + N * T
        g = torch.Generator(device=dev).manual_seed(7)
        k = torch.randn(B, L, H * hd, device=dev, generator=g).to(torch.bfloat16)
        v = torch.randn(B, L, H * hd, device=dev, generator=g).to(torch.bfloat16)
        q = torch.randn(B, L, H * hd, device=dev, generator=g)
        kn = k.float().reshape(B, L, H, hd).norm(dim=-1).max()
        q = (q * (40.0 / float(q.reshape(B, L, H, hd).norm(dim=-1).max() * kn))).to(torch.bfloat16)   # prescaled, |q||k| <= ~40 < 56
        bound = float(q.float().reshape(B, L, H, hd).norm(dim=-1).max() * kn) * 1.01
        vt = torch.zeros(B, H, hd, (L + 63) // 64 * 64, dtype=torch.bfloat16, device=dev)
        _C.v_transpose(v, vt, H, hd)
        out = torch.empty_like(q)
        ws_full = _C.attention_workspace(dev)
        ws_win = _C.attention_window_workspace(B, H, L, hd, dev)
        tables = {w: mmdit.attention_window_table(Lt, N * T, N, w) for w in s["windows"]}
        arms = {"full": lambda: _C.attention_fwd(q, k, vt, out, H, hd, hd ** -0.5, q_prescaled=True, workspace=ws_full, score_bound=bound)}
        for w, t in tables.items():
            arms[f"W{w}"] = (lambda t=t: _C.attention_fwd_window(q, k, vt, out, H, hd, hd ** -0.5, n_prefix=Lt, windows=t, q_prescaled=True,
                                                                 score_bound=bound, workspace=ws_win))
        for fn in arms.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {n_: [] for n_ in arms}
        for _ in range(a.repeats):
            for n_, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(s["inner"]):
                    fn()
                e1.record()
                e1.synchronize()
                ms[n_].append(e0.elapsed_time(e1) / s["inner"])
        med = {n_: statistics.median(x) for n_, x in ms.items()}
        rows_unit = _C.attention_launch_shape(B, H, L, 1, L, hd, bound, ws_full.numel()) if hasattr(_C, "attention_launch_shape") else None
        for n_ in arms:
            frac = 1.0 if n_ == "full" else mmdit.window_tile_fraction(tables[int(n_[1:])], Lt, N * T)
            ratio = med[n_] / med["full"]
            emit(dict(what="attn_window_time", shape=s["name"], B=B, H=H, hd=hd, L_txt=Lt, frame_tokens=N, frames=T, arm=n_,
                      window_frames=None if n_ == "full" else int(n_[1:]), repeats=a.repeats, calls_per_timing=s["inner"],
                      ms=[round(x, 4) for x in ms[n_]], median_ms=round(med[n_], 4), spread_ms=round(max(ms[n_]) - min(ms[n_]), 4),
                      tile_fraction=round(frac, 4), time_ratio=round(ratio, 4), time_ratio_over_tile_fraction=round(ratio / frac, 4),
                      full_call_launch_shape=str(rows_unit) if n_ == "full" else None, score_bound=round(bound, 3)))
        del q, k, v, vt, out


if __name__ == "__main__":
    main()
