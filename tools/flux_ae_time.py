"""Time the Flux 2-D autoencoder (open_sora_amd.flux_ae, shipped widths ch 128, ch_mult [1, 2, 4, 4], bf16, B = 1) on the GPU:
decode (and encode) at 576 x 1024 and 256 x 256, against a plain-PyTorch decoder / encoder of the same weights
(tests/flux_ae_restatement.py with use_torch_conv: F.conv2d / F.group_norm / SDPA) in bf16 and fp32.

FLOPs are counted algorithmically, not from what the kernels execute:
    conv      2 * Cin * Cout * k^2 * Ho * Wo          (every conv, 1 x 1 included; Cin unpadded)
    attention 4 * S^2 * C + 8 * S * C^2               (mid block: QK^T and P.V, plus the q / k / v / proj_out projections)
GroupNorm, SiLU and the boundary conversions count zero.  Peak = 2.5 PFLOP/s bf16 dense.

    python tools/flux_ae_time.py [--iters 10] [--no-encode] [--no-torch]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import flux_ae_restatement as R  # noqa: E402

PEAK = 2.5e15
BF = torch.bfloat16


def ae_flops(cfg: dict, H: int, W: int, decode: bool) -> tuple[float, float]:
    """(total, 3 x 3 stride-1 conv part) FLOPs of one decode to / encode of an H x W image"""
    ch, mult, nrb, zc = cfg["ch"], cfg["ch_mult"], cfg["num_res_blocks"], cfg["z_channels"]
    n = len(mult)
    tot = [0.0, 0.0]

    def conv(ci, co, k, ho, wo, s1=True):
        f = 2.0 * ci * co * k * k * ho * wo
        tot[0] += f
        if k == 3 and s1:
            tot[1] += f

    def res(ci, co, h, w):
        conv(ci, co, 3, h, w)
        conv(co, co, 3, h, w)
        if ci != co:
            conv(ci, co, 1, h, w)

    def mid(c, h, w):
        res(c, c, h, w)
        S = h * w
        tot[0] += 4.0 * S * S * c + 8.0 * S * c * c
        res(c, c, h, w)

    if decode:
        h, w = H >> (n - 1), W >> (n - 1)
        c = ch * mult[-1]
        conv(zc, c, 3, h, w)
        mid(c, h, w)
        for lvl in reversed(range(n)):
            co = ch * mult[lvl]
            for _ in range(nrb + 1):
                res(c, co, h, w)
                c = co
            if lvl != 0:
                h, w = 2 * h, 2 * w
                conv(c, c, 3, h, w)
        conv(c, cfg["out_ch"], 3, h, w)
    else:
        h, w = H, W
        conv(cfg["in_channels"], ch, 3, h, w)
        c = ch
        for lvl in range(n):
            co = ch * mult[lvl]
            for _ in range(nrb):
                res(c, co, h, w)
                c = co
            if lvl != n - 1:
                h, w = h // 2, w // 2
                conv(c, c, 3, h, w, s1=False)
        mid(c, h, w)
        conv(c, 2 * zc, 3, h, w)
    return tot[0], tot[1]


def timed(fn, iters: int) -> float:
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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sizes", default="576x1024,256x256")
    ap.add_argument("--no-encode", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()

    from open_sora_amd import _C, flux_ae

    dev = "cuda:0"
    torch.cuda.set_device(0)
    cfg = R.SHIPPED
    m = flux_ae.AutoEncoderFlux(from_pretrained=None, device_map=dev, torch_dtype=BF, **cfg)
    sd = R.make_state_dict(m)
    m.load_state_dict(sd, strict=True)
    m.sample = False
    sd_b = {k: v.to(dev, BF) for k, v in sd.items()}
    sd_f = {k: v.to(dev) for k, v in sd.items()}
    n = len(cfg["ch_mult"])
    for size in a.sizes.split(","):
        H, W = (int(s) for s in size.split("x"))
        z = torch.randn(1, cfg["z_channels"], 1, H >> (n - 1), W >> (n - 1), device=dev).to(BF)
        x = (0.5 * torch.randn(1, 3, 1, H, W, device=dev)).to(BF)
        jobs = [("decode", True, lambda: m.decode(z), lambda sd_: R.decode(sd_, cfg, z.to(sd_["decoder.conv_in.weight"].dtype)))]
        if not a.no_encode:
            jobs.append(("encode", False, lambda: m.encode(x), lambda sd_: R.encode_mode(sd_, cfg, x.to(sd_["encoder.conv_in.weight"].dtype))))
        for what, dec, ours, plain in jobs:
            fl, fl3 = ae_flops(cfg, H, W, dec)
            with torch.inference_mode():
                ms = timed(ours, a.iters)
                # per-conv events (one profiled call): the 3 x 3 stride-1 convolutions' own time
                _C.PROFILE_CONV = []
                ours()
                torch.cuda.synchronize()
                prof, _C.PROFILE_CONV = _C.PROFILE_CONV, None
                conv_ms = sum(e0.elapsed_time(e1) for e0, e1, _ in prof)
                row = dict(what=what, size=f"{H}x{W}", ms=round(ms, 3), tflops=round(fl / ms / 1e9, 1),
                           frac_peak=round(fl / ms / 1e-3 / PEAK, 3), gflop=round(fl / 1e9, 1), conv_launches=len(prof),
                           conv_ms=round(conv_ms, 3), conv3x3_s1_gflop=round(fl3 / 1e9, 1))
                if not a.no_torch:
                    R.use_torch_conv(True)     # the comparator is the plain-PyTorch decoder: F.conv2d in the weights' dtype
                    try:
                        for dt_name, sd_ in (("bf16", sd_b), ("fp32", sd_f)):
                            row[f"torch_{dt_name}_ms"] = round(timed(lambda: plain(sd_), max(2, a.iters // 2)), 3)
                    finally:
                        R.use_torch_conv(False)
            print(json.dumps(row), flush=True)
            print(f"  {what} {H}x{W}: {ms:.3f} ms = {fl / ms / 1e9:.1f} TFLOP/s = {fl / ms / 1e-3 / PEAK:.3f} of 2.5 PFLOP/s"
                  + ("" if a.no_torch else f"; plain torch bf16 {row['torch_bf16_ms']:.3f} ms, fp32 {row['torch_fp32_ms']:.3f} ms"),
                  flush=True)


if __name__ == "__main__":
    main()
