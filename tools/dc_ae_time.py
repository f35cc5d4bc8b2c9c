"""Time the Video DC-AE decoder, or with --encode the encoder (open_sora_amd.dc_ae, dc-ae-f32t4c128, bf16, B = 1), on the GPU with
device events after a warm-up:

  tile   one full tile, latent [1, 128, 8, 8, 8] -> 32 x 256 x 256;
  tiled  (--tiled) the tiled decode of the shipped configuration, latent [1, 128, 32, 24, 24] -> 128 x 768 x 768;
  and, for comparison, the plain-PyTorch decoder of the same weights (tests/dc_ae_restatement.py: F.conv3d, matmul) in bf16 on
  the same GPU in the same process (--no-torch skips it).

  --encode: the same three for the encoder: one tile [1, 3, 32, 256, 256] -> latent 8 x 8 x 8, the tiled encode of
  [1, 3, 128, 768, 768], and tests/dc_ae_enc_restatement.py in bf16; the strided downsample convs are reported on their own.

FLOPs are counted algorithmically.  The 3 x 3 x 3 convolutions' own time comes from one profiled call with an event pair around
every conv launch (_C.PROFILE_CONV); their fraction of the 2.5 PFLOP/s bf16 peak is 2 * Cin * Cout * 27 * voxels / time / peak.

    python tools/dc_ae_time.py [--encode] [--iters 5] [--tiled] [--no-torch] [--out profiles/dc_ae_time.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import dc_ae_enc_restatement as RE  # noqa: E402
from tests import dc_ae_restatement as R  # noqa: E402

PEAK = 2.5e15
BF = torch.bfloat16


def timed(fn, iters: int, warmup: int = 1) -> float:
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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--encode", action="store_true", help="time the encoder instead of the decoder")
    ap.add_argument("--tiled", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--once", action="store_true", help="one un-timed tile decode and exit (the run a kernel trace wraps)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from open_sora_amd import _C, dc_ae

    dev = "cuda:0"
    torch.cuda.set_device(0)
    if a.encode:
        return encode_main(a, _C, dc_ae, dev)
    m = dc_ae.DC_AE("dc-ae-f32t4c128", device_map=dev, torch_dtype=BF, from_scratch=True, use_spatial_tiling=True,
                    use_temporal_tiling=True)
    sd = R.make_state_dict(R.param_shapes(R.SHIPPED), seed=1)
    m.load_state_dict(sd)
    z = torch.randn(1, 128, 8, 8, 8, device=dev).to(BF)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "a") as f:
                f.write(json.dumps(row) + "\n")

    with torch.inference_mode():
        if a.once:
            m.decode(z)
            torch.cuda.synchronize()
            m.decode(z)
            torch.cuda.synchronize()
            return
        ms = timed(lambda: m.decode(z), a.iters)
        ksizes = []
        plain_conv = _C.conv3d_zp

        def tagged(x, w, bias, out, ksize, *args, **kw):
            ksizes.append(ksize)
            return plain_conv(x, w, bias, out, ksize, *args, **kw)

        _C.PROFILE_CONV, _C.conv3d_zp = [], tagged
        try:
            m.decode(z)
            torch.cuda.synchronize()
        finally:
            prof, _C.PROFILE_CONV, _C.conv3d_zp = _C.PROFILE_CONV, None, plain_conv
        c3 = [(e0.elapsed_time(e1), fl) for (e0, e1, fl), k in zip(prof, ksizes) if k == 3]
        c3_ms, c3_fl = sum(t for t, _ in c3), sum(f for _, f in c3)
        row = dict(what="tile", latent=[1, 128, 8, 8, 8], video=[32, 256, 256], ms=round(ms, 3), conv3x3x3_launches=len(c3),
                   conv3x3x3_ms=round(c3_ms, 3), conv3x3x3_tflop=round(c3_fl / 1e12, 2),
                   conv3x3x3_frac_peak=round(c3_fl / (c3_ms * 1e-3) / PEAK, 3))
        if not a.no_torch:
            sd_b = {k: v.to(dev, BF) for k, v in sd.items()}
            t_ms = timed(lambda: R.decode(sd_b, R.SHIPPED, z), max(1, a.iters // 2))
            row["torch_bf16_ms"] = round(t_ms, 3)
            row["ratio_torch_over_hip"] = round(t_ms / ms, 2)
            del sd_b
        emit(row)
        if a.tiled:
            zt = torch.randn(1, 128, 32, 24, 24, device=dev).to(BF)
            ms = timed(lambda: m.decode(zt), 1)
            out = m.decode(zt)
            emit(dict(what="tiled", latent=list(zt.shape), video=list(out.shape[2:]), ms=round(ms, 1)))


def encode_main(a, _C, dc_ae, dev):
    m = dc_ae.DC_AE_with_encoder("dc-ae-f32t4c128", device_map=dev, torch_dtype=BF, from_scratch=True, use_spatial_tiling=True,
                                 use_temporal_tiling=True)
    sd = dict(R.make_state_dict(RE.enc_param_shapes(RE.SHIPPED), seed=1))
    sd.update(R.make_state_dict(R.param_shapes(R.SHIPPED), seed=1))
    m.load_state_dict(sd)
    x = torch.randn(1, 3, 32, 256, 256, device=dev).to(BF)

    def emit(row):
        print(json.dumps(row), flush=True)
        if a.out:
            with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "a") as f:
                f.write(json.dumps(row) + "\n")

    with torch.inference_mode():
        if a.once:
            m.encode(x)
            torch.cuda.synchronize()
            m.encode(x)
            torch.cuda.synchronize()
            return
        ms = timed(lambda: m.encode(x), a.iters)
        kinds = []
        plain, plain_s = _C.conv3d_zp, _C.conv3d_zp_strided

        def tagged(x_, w, bias, out, ksize, *args, **kw):
            kinds.append("k3" if ksize == 3 else "k1")
            return plain(x_, w, bias, out, ksize, *args, **kw)

        def tagged_s(*args, **kw):
            kinds.append("strided")
            return plain_s(*args, **kw)

        _C.PROFILE_CONV, _C.conv3d_zp, _C.conv3d_zp_strided = [], tagged, tagged_s
        try:
            m.encode(x)
            torch.cuda.synchronize()
        finally:
            prof, _C.PROFILE_CONV, _C.conv3d_zp, _C.conv3d_zp_strided = _C.PROFILE_CONV, None, plain, plain_s
        row = dict(what="encode tile", video=[32, 256, 256], latent=[1, 128, 8, 8, 8], ms=round(ms, 3))
        for kind, tag in (("k3", "conv3x3x3"), ("strided", "strided")):
            sel = [(e0.elapsed_time(e1), fl) for (e0, e1, fl), k in zip(prof, kinds) if k == kind]
            t, fl = sum(v for v, _ in sel), sum(f for _, f in sel)
            row.update({tag + "_launches": len(sel), tag + "_ms": round(t, 3), tag + "_tflop": round(fl / 1e12, 2),
                        tag + "_frac_peak": round(fl / (t * 1e-3) / PEAK, 3)})
        if not a.no_torch:
            sd_b = {k: v.to(dev, BF) for k, v in sd.items() if k.startswith("encoder.")}
            t_ms = timed(lambda: RE.encode(sd_b, RE.SHIPPED, x), max(1, a.iters // 2))
            row["torch_bf16_ms"] = round(t_ms, 3)
            row["ratio_torch_over_hip"] = round(t_ms / ms, 2)
            del sd_b
        emit(row)
        if a.tiled:
            xt = torch.randn(1, 3, 128, 768, 768, device=dev).to(BF)
            ms = timed(lambda: m.encode(xt), 1)
            out = m.encode(xt)
            emit(dict(what="encode tiled", video=list(xt.shape[2:]), latent=list(out.shape), ms=round(ms, 1)))


if __name__ == "__main__":
    main()
