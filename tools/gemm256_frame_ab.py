#!/usr/bin/env python
"""Parent library against new library for the 256-row GEMM frame (csrc/tile256.h, gemm256x.hip's tile walk, the fp8 kernel on the shared
epilogue): outputs must be EQUAL byte for byte; timing legs are interleaved by the caller, one library per process.

  OSK_ALT_LIB=<libosk_hip.so> python tools/gemm256_frame_ab.py dump <file.json>  seeded cases through ONE library -> SHA-256 of every output
  python tools/gemm256_frame_ab.py compare <a.json> <b.json>                     exit 1 unless every case is byte-identical
  OSK_ALT_LIB=... python tools/gemm256_frame_ab.py time                          one JSON line: median ms of the timed Linears

Each case runs on the kernel named: osk_gemm_tile_override forces the bf16 tile (2: gemm256x, 1: gemm256p); groups run on gemm256x only, and
so does the pair at the shape used here (osk_gemm_bf16_pair's estimate, gemm_bf16.hip, takes one launch for
(53 row tiles x 14 column tiles: 3 rounds of the chip against 3 + 1)); the fp8 tile width follows from the shape (gemm_fp8.hip: 256 wide only where 256-wide tiles save a round of the chip)."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import _altlib

def rnd(shape, seed, std=1.0, dtype=None):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * std).to(dtype or torch.bfloat16).cuda()


def linear(C, B, L, N, K, seed, gelu_from=None, gated=False, out_f32=False):
    import torch
    a, w = rnd((B, L, K), seed), rnd((N, K), seed + 1, K ** -0.5)
    bias = rnd((N,), seed + 2, 0.2, torch.float32)
    if gated:
        out, gate = rnd((B, L, N), seed + 3), rnd((B, N), seed + 4, 0.5, torch.float32)
        return C.gemm(a, w, bias, out, res=out, gate=gate, gate_batch_stride=gate.stride(0))
    out = torch.empty(B, L, N, dtype=torch.float32 if out_f32 else torch.bfloat16, device="cuda")
    return C.gemm(a, w, bias, out, gelu_from=gelu_from)


def pair(C, gated):
    import torch
    B, Li, Lt, N, K = 3, 4000, 512, 3456, 1152
    outs, ds = [], []
    for i, L in enumerate((Li, Lt)):
        d = dict(a=rnd((B, L, K), 300 + i), w=rnd((N, K), 302 + i, K ** -0.5), bias=rnd((N,), 304 + i, 0.2, torch.float32))
        if gated:
            d["out"] = rnd((B, L, N), 306 + i)
            d["res"], d["gate"] = d["out"], rnd((B, N), 308 + i, 0.5, torch.float32)
            d["gate_batch_stride"] = N
        else:
            d["out"] = torch.empty(B, L, N, dtype=torch.bfloat16, device="cuda")
        ds.append(d)
        outs.append(d["out"])
    C.gemm_pair(ds[0], ds[1])
    return outs


def skip_and_vt(C):
    """tests/test_gpu_kernels.py::test_gemm_group_skip_range_and_block_packs, first group"""
    import torch
    H, hd, B, L = 16, 72, 2, 128 + 1100
    D, R = H * hd, 4 * H * hd
    xm, w1, b1 = rnd((B, L, D), 211), rnd((3 * D + R, D), 212, D ** -0.5), rnd((3 * D + R,), 213, 0.2, torch.float32)
    y = torch.full((B, L, 3 * D + R), 3.0, dtype=torch.bfloat16, device="cuda")
    vt = torch.zeros(B, H, hd, (L + 63) // 64 * 64, dtype=torch.bfloat16, device="cuda")
    assert C.gemm_group([dict(a=xm, w=w1, bias=b1, out=y, gelu_from=3 * D, skip=(2 * D, D)),
                         dict(x=xm, w=w1[2 * D: 3 * D], bias=b1[2 * D: 3 * D], vt=vt, vt_pos=0, hd=hd)])
    return [y, vt]


def vt_walk(C, single):
    """tests/test_gpu_kernels.py::test_gemm_group_vt_workgroups_walk_several_tiles"""
    import torch
    hd, H, K = 64, 16, 128
    B, streams = (2, [(0, 8400)]) if single else (1, [(128, 16500), (0, 128)])
    L = sum(n for _, n in streams)
    x = rnd((B, L, K), 231)
    vt = torch.full((B, H, hd, (L + 63) // 64 * 64 + 64), 7.0, dtype=torch.bfloat16, device="cuda")
    assert C.gemm_group([dict(x=x[:, r0: r0 + n], w=rnd((H * hd, K), 232 + i, K ** -0.5), bias=rnd((H * hd,), 236 + i, 0.3, torch.float32),
                              vt=vt, vt_pos=64 + r0, hd=hd) for i, (r0, n) in enumerate(streams)])
    return vt


def fp8(C, B, L, N, K, seed, bias=True, gelu_from=None, gated=False, out_f32=False, row_pad=0):
    import torch
    a8, sa = C.quantize_rows_fp8(rnd((B, L, K), seed))
    w8, sw = C.quantize_rows_fp8(rnd((N, K), seed + 1, K ** -0.5))
    b = rnd((N,), seed + 2, 0.1, torch.float32) if bias else None
    dt = torch.float32 if out_f32 else torch.bfloat16
    full = rnd((B, L, N + row_pad), seed + 3, dtype=dt)          # row_pad = 4: rows 8-byte but not 16-byte aligned
    out = full[:, :, :N]
    if gated:
        gate = rnd((B, N), seed + 4, 0.5, torch.float32)
        C.gemm_fp8(a8, sa, w8, sw, b, out, res=out, gate=gate, gate_batch_stride=N)
    else:
        C.gemm_fp8(a8, sa, w8, sw, b, out, gelu_from=gelu_from)
    return full


def cases(C):
    ov = C.lib.osk_gemm_tile_override
    ov(2)                                                           # ---- gemm256x Linear
    yield "x_1x256_256_64", linear(C, 1, 256, 256, 64, 100)
    yield "x_2x300_384_192", linear(C, 2, 300, 384, 192, 110)
    yield "x_1x40000_512_64", linear(C, 1, 40000, 512, 64, 120)
    yield "x_3x5000_2304_192_gelu1000", linear(C, 3, 5000, 2304, 192, 130, gelu_from=1000)
    yield "x_3x9000_1152_256_gated", linear(C, 3, 9000, 1152, 256, 140, gated=True)
    yield "x_1x1000_520_256_f32", linear(C, 1, 1000, 520, 256, 150, out_f32=True)
    ov(-1)                                                          # ---- gemm256x packs
    yield "pair_plain", pair(C, False)
    yield "pair_gated", pair(C, True)
    yield "skip_and_vt", skip_and_vt(C)
    yield "vt_walk_single", vt_walk(C, True)
    yield "vt_walk_img_txt", vt_walk(C, False)
    ov(1)                                                           # ---- gemm256p
    yield "p_2x20000_640_128_gelu384", linear(C, 2, 20000, 640, 128, 160, gelu_from=384)
    yield "p_1x33000_1000_320_gated", linear(C, 1, 33000, 1000, 320, 170, gated=True)
    ov(-1)                                                          # ---- fp8: N = 6152 at M = 2000 -> 256-wide tiles, else 128-wide
    for wide, (L, N) in (("n128", (300, 392)), ("n256", (1000, 6152))):     # B = 2: ragged M and N, a 256-row tile straddles the batches
        yield f"fp8_{wide}_bf16", fp8(C, 2, L, N, 256, 400)
        yield f"fp8_{wide}_f32_nobias", fp8(C, 2, L, N, 256, 410, bias=False, out_f32=True)
        yield f"fp8_{wide}_gelu_inside_tile", fp8(C, 2, L, N, 256, 420, gelu_from=N // 2 + 13)
        yield f"fp8_{wide}_gated_aligned", fp8(C, 2, L, N, 256, 430, gated=True)
        yield f"fp8_{wide}_gated_row_stride_8B", fp8(C, 2, L, N, 256, 440, gated=True, row_pad=4)
        yield f"fp8_{wide}_nobias_gelu", fp8(C, 2, L, N, 128, 450, bias=False, gelu_from=128)


def main():
    mode = sys.argv[1]
    if mode == "compare":
        a, b = json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))
        assert a.keys() == b.keys()
        bad = [k for k in a if a[k] != b[k]]
        print(json.dumps({"cases": len(a), "different": bad}))
        sys.exit(1 if bad else 0)
    lib_path = _altlib.install()
    import torch
    from open_sora_amd import _C as C
    if mode == "dump":
        out = {}
        for name, res in cases(C):
            out[name] = [hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()      # (whole storage rows,
                         for t in (res if isinstance(res, (list, tuple)) else [res])]                              # padding included)
        json.dump(out, open(sys.argv[2], "w"), indent=1)
        print(json.dumps({"lib": lib_path or "shipped", "cases": len(out)}))
        return
    assert mode == "time"
    rec = {"lib": lib_path or "shipped"}

    def med(fn):
        for _ in range(5):
            fn()
        ms = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / 20)
        return round(sorted(ms)[3], 4)

    for M, N, K in ((50688, 4608, 1152), (49152, 1152, 1152)):
        a, w, b = rnd((1, M, K), 1), rnd((N, K), 2, K ** -0.5), rnd((N,), 3, 0.2, torch.float32)
        out = torch.empty(1, M, N, dtype=torch.bfloat16, device="cuda")
        rec[f"bf16_{M}x{N}x{K}_ms"] = med(lambda: C.gemm(a, w, b, out))
    M, N, K = 49152, 4608, 1152
    a8, sa = C.quantize_rows_fp8(rnd((1, M, K), 4))
    w8, sw = C.quantize_rows_fp8(rnd((N, K), 5, K ** -0.5))
    b, out = rnd((N,), 6, 0.2, torch.float32), torch.empty(1, M, N, dtype=torch.bfloat16, device="cuda")
    rec[f"fp8_{M}x{N}x{K}_ms"] = med(lambda: C.gemm_fp8(a8, sa, w8, sw, b, out, gelu_from=0))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
