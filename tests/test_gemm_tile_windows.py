"""CPU: the support condition of the large-tile GEMM kernels is per TILE, not per tensor (csrc/tile256.h, the addressing rule).

osk_gemm_tile_choice_strided reports the kernel osk_gemm_bf16 launches for given operand strides from the dispatch's own code and
launches nothing, so the condition can be walked here without a GPU or any memory: every 256-row window of A and of W has to lie
within 2^32 - 1 bytes of its own origin -- a batch jump inside the window included, forwards or backwards -- while the operands
themselves may span more than 4 GiB.  Where the condition fails the dispatch keeps the 128 x 128 kernel (kind 0)."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIB4 = 1 << 32


def _lib():
    from open_sora_amd import _C

    return _C


def test_strided_entry_is_declared_bound_and_wrapped():
    C = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "osk.h")).read(), flags=re.S)
    m = re.search(r"int\s+osk_gemm_tile_choice_strided\s*\(([^)]*)\)", src)
    assert m, "include/osk.h does not declare osk_gemm_tile_choice_strided"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.rsplit(" ", 1)[0] for p in params] == ["int", "int", "int", "int64_t", "int64_t", "int", "int64_t"], params
    i32, i64 = C._i32, C._i64
    assert C.SIGNATURES["osk_gemm_tile_choice_strided"] == [i32, i32, i32, i64, i64, i32, i64]
    assert C.lib.osk_abi_version() == 2                                   # an additive entry: the version stays
    # the wrapper reads shapes and strides only: tensors without storage will do
    a = torch.empty_strided((3, 16896, 1152), (16896 * 1152, 1152, 1), dtype=torch.bfloat16, device="meta")
    w = torch.empty_strided((1152, 1152), (1152, 1), dtype=torch.bfloat16, device="meta")
    assert C.gemm_tile_kind(a, w) == C.lib.osk_gemm_tile_choice(3 * 16896, 1152, 1152) == 2


def test_window_condition_through_the_reporting_entry():
    C = _lib()
    pick, strided = C.lib.osk_gemm_tile_choice, C.lib.osk_gemm_tile_choice_strided

    def same(M, N, K, abs_, ars, arpb, wrs):
        want = pick(M, N, K)
        assert want in (1, 2), (M, N, K, want)                            # (a case that proves nothing if the estimate says 0)
        assert strided(M, N, K, abs_, ars, arpb, wrs) == want, (M, N, K, abs_, ars, arpb, wrs)

    def falls_back(M, N, K, abs_, ars, arpb, wrs):
        assert pick(M, N, K) in (1, 2)
        assert strided(M, N, K, abs_, ars, arpb, wrs) == 0, (M, N, K, abs_, ars, arpb, wrs)

    # ---- below the old limit: contiguous and column-slice operands, several batches
    same(3 * 16896, 1152, 1152, 16896 * 1152, 1152, 16896, 1152)
    same(2 * 3000, 3072, 15360, 3000 * 21504, 21504, 3000, 15360)
    # ---- above the old limit with a fitting window
    M, ars = 100096, 21504                                                # the fused buffer y of an 11B single-stream block
    assert (M - 1) * ars * 2 > GIB4
    same(M, 3072, 15360, M * ars, ars, M, 15360)                          # linear2
    same(M, 256, 128, M * ars, ars, M, 128)
    same(229632, 3072, 15360, 229632 * ars, ars, 229632, 15360)           # the reference's 768 px table, 1 GPU
    same(3 * 230912, 3072, 3072, 230912 * 3072, 3072, 230912, 3072)       # CFG batch 3: contiguous [B L, 3072] is 4.26 GB
    wrs = (1 << 22) + 64                                                  # W rows 8 MiB + 128 bytes apart: row 512 starts past 4 GiB
    assert 519 * wrs * 2 > GIB4 and 255 * wrs * 2 + 256 < GIB4
    same(512, 520, 128, 0, 128, 512, wrs)
    same(512, 512, 128, 0, 128, 512, wrs)                                 # (512 rows: the last row still starts below 4 GiB)
    same(1024, 256, 128, (1 << 31) + 4096, 128, 512, 128)                 # batches 4 GiB + 8 KiB apart, no tile across the jump
    same(1024, 256, 128, -((1 << 31) + 4096), 128, 512, 128)              # ... and the second batch BELOW the first
    # ---- a window too wide for 32 bits: a row stride past 2^23 elements (row 255 of a tile starts 255 strides x 2 bytes from row 0:
    # 255 * (2^23 + 2^16) * 2 = 4.31e9 > 2^32)
    wide = (1 << 23) + (1 << 16)
    falls_back(1024, 256, 128, 0, wide, 1024, 128)
    falls_back(1024, 256, 128, 0, 128, 1024, wide)
    falls_back(1024, 256, 128, 0, 1 << 24, 1024, 128)
    same(1024, 256, 128, 0, 1 << 22, 1024, 1 << 22)                       # half of it fits
    # ---- a straddled batch jump: 384 rows per batch put tile 1 (rows 256 .. 383 of batch 0, rows 0 .. 127 of batch 1) across it.  Its
    # window runs from row 256 of batch 0 to row 127 of batch 1: batch stride - 129 row strides, + K.  Forwards, a batch stride of
    # 2^31 + 4096 elements is therefore 24 KiB INSIDE the limit (the tile starts 64 KiB into batch 0); 2^31 + 32768 is 32 KiB past it.
    # Backwards the window is batch stride + 383 row strides.
    same(768, 256, 128, (1 << 31) + 4096, 128, 384, 128)
    falls_back(768, 256, 128, (1 << 31) + 32768, 128, 384, 128)
    falls_back(768, 256, 128, -((1 << 31) + 4096), 128, 384, 128)         # backwards
    same(768, 256, 128, 1 << 30, 128, 384, 128)                           # a jump of 2 GiB fits, either way
    same(768, 256, 128, -(1 << 30), 128, 384, 128)
    same(2000 * 100, 256, 128, 1 << 24, 128, 100, 128)                    # 100-row batches 32 MiB apart (64 GB in all): a tile holds 3-4 of them
    falls_back(2000 * 100, 256, 128, 1 << 30, 128, 100, 128)              # ... 2 GiB apart: three of them do not fit
    # ---- the shapes the large tiles never took stay where they were, and bad arguments are refused
    assert strided(255, 256, 128, 0, 128, 255, 128) == 0
    assert strided(1024, 256, 100, 0, 128, 1024, 128) < 0                 # K % 64
    assert strided(1024, 256, 128, 0, 129, 1024, 128) < 0                 # stride % 8
    assert strided(1024, 256, 128, 0, 128, 0, 128) < 0


def test_override_is_seen_by_both_reporting_entries():
    C = _lib()
    try:
        for kind in (0, 1, 2):
            assert C.lib.osk_gemm_tile_override(kind) == 0
            assert C.lib.osk_gemm_tile_choice_strided(100096, 256, 128, 0, 21504, 100096, 128) == kind
            assert C.lib.osk_gemm_tile_choice_strided(768, 256, 128, (1 << 31) + 32768, 128, 384, 128) == 0   # never past the condition
    finally:
        C.lib.osk_gemm_tile_override(-1)
