"""GPU: the large-tile GEMM kernels on operands that span more than 4 GiB.

The 256-row tile kernels (gemm256x Linear and V^T walks, gemm256p, the fp8 gemm256) address every tile relative to its own origin
(csrc/tile256.h): one tile's 256-row window has to fit their 32-bit lane offsets, the operand does not.  Every case here puts an
operand past 4 GiB -- a 4.3 - 4.4 GB buffer from torch.empty of which only the columns the GEMM reads are written, K = 128 / 256 and
N = 256 / 384 keep the arithmetic tiny -- and checks
  * rows of the first tile, a middle tile and the last tile (which holds the 4 GiB crossing) against an f64 product of the same bf16 /
    e4m3 inputs, with the tolerances of the GEMM cases of tests/test_gpu_kernels.py (bf16_ulp_close rel 2^-7, abs 2e-3; 3e-3 with the
    gate epilogue) and tests/test_gpu_fp8.py (rel 2^-7, abs 2e-3);
  * the COMPLETE output bit for bit against the same problem run from a small contiguous copy of the same rows on the same tile
    kernel (osk_gemm_tile_choice_strided reports it for both): a wrong row anywhere shows.
"""
import pytest
import torch

from tests.test_gpu_kernels import BF, DEV, bf16_ulp_close

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
GIB4 = 1 << 32
YS = 21504                      # row stride of the fused buffer y of an 11B single-stream block: 7 * 3072
M_Y = 100096                    # 391 row tiles; row 99,864 -- inside the last tile -- starts past 4 GiB


def _need_memory(gb=12):
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < gb * 10 ** 9:
        pytest.skip(f"{free / 1e9:.1f} GB of device memory free: the > 4 GiB operands of this test need {gb} GB")


def _randn(shape, seed, std=1.0, dtype=BF):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV, dtype=torch.float32) * std).to(dtype)


def _sample_rows(M):
    """rows of the first tile, a middle tile and the last tile, their first and last rows included"""
    pick = lambda lo, hi: [lo, lo + 1, lo + 77, (lo + hi) // 2, hi - 2, hi - 1]
    mid = (M // 512) * 256
    last = (M - 1) // 256 * 256
    return torch.tensor(sorted(set(pick(0, 256) + pick(mid, mid + 256) + pick(last, M))), device=DEV)


def _f64_rows(a_rows, w, bias, res_rows=None, gate=None):
    v = a_rows.double().cpu() @ w.double().cpu().T + bias.double().cpu()
    if gate is not None:
        v = res_rows.double().cpu() + gate.double().cpu() * v
    return v


@pytest.fixture
def y_buffer():
    """the > 4 GiB fused buffer [1, M_Y, 21504] bf16 (uninitialised: the tests write the columns they read)"""
    _need_memory()
    buf = torch.empty(M_Y * YS, dtype=BF, device=DEV)
    assert buf.numel() * 2 > GIB4
    yield buf
    del buf
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ case 1: A past 4 GiB by row count
@pytest.mark.parametrize("gated,N", [(False, 256), (True, 384)], ids=["plain_n256", "gate_residual_n384"])
def test_a_past_4gib_by_row_count(hip_lib, y_buffer, gated, N):
    """y-shaped: A = y[:, :, 6144 : 6144 + K], C = a column slice of a second view of the same buffer (as linear2 / linear1 use it),
    plain and gate * x + residual in place (N = 384: an N-edge tile); by the estimate and on each forced large-tile kernel."""
    K, M = 128, M_Y
    y = y_buffer.view(1, M, YS)
    a = y[:, :, 6144: 6144 + K]
    a.copy_(_randn((1, M, K), 11))
    c = y_buffer.view(1, M, YS)[:, :, :N]
    w = _randn((N, K), 12, std=K ** -0.5)
    bias = _randn((N,), 13, std=0.1, dtype=torch.float32)
    gate = _randn((1, N), 14, std=0.5, dtype=torch.float32) if gated else None
    res0 = _randn((1, M, N), 15) if gated else None
    a_small = a.contiguous()
    rows = _sample_rows(M)
    assert (M - 1) * YS * 2 > GIB4 > (M - 256) * YS * 2, "the last tile straddles the 4 GiB crossing"

    def run(a_, out):
        if gated:
            out.copy_(res0)
            hip_lib.gemm(a_, w, bias, out, res=out, gate=gate, gate_batch_stride=gate.stride(0))
        else:
            hip_lib.gemm(a_, w, bias, out)
        return out

    # by the estimate: the kernel the shape gets anywhere else
    want = hip_lib.lib.osk_gemm_tile_choice(M, N, K)
    assert want in (1, 2)
    assert hip_lib.gemm_tile_kind(a, w) == hip_lib.gemm_tile_kind(a_small, w) == want
    try:
        for forced in (-1, 2, 1):
            assert hip_lib.lib.osk_gemm_tile_override(forced) == 0
            kind = hip_lib.gemm_tile_kind(a, w)
            assert kind == hip_lib.gemm_tile_kind(a_small, w) == (want if forced < 0 else forced)
            got = run(a, c)
            ref = run(a_small, torch.empty(1, M, N, dtype=BF, device=DEV))
            torch.cuda.synchronize()
            assert torch.equal(got, ref), f"tile kind {kind}: the strided > 4 GiB run differs from the contiguous copy"
            v = _f64_rows(a_small[0, rows], w, bias, res0[0, rows] if gated else None, gate)
            bf16_ulp_close(got[0, rows].float().cpu(), v.float().bfloat16().float(), rel=2 ** -7, abs_=3e-3 if gated else 2e-3)
    finally:
        hip_lib.lib.osk_gemm_tile_override(-1)


# ------------------------------------------------------------------------------------------------ case 2: A past 4 GiB by batch stride
@pytest.mark.parametrize("L,extra,fits", [(512, 4096, True), (384, 4096, True), (384, 32768, False)],
                         ids=["512_rows_per_batch", "384_rows_straddling_fits", "384_rows_straddling_too_wide"])
def test_a_past_4gib_by_batch_stride(hip_lib, L, extra, fits):
    """Two batches 2^31 + extra elements apart.  512 rows per batch: no tile crosses the jump.  384 rows per batch: tile 1 holds rows
    256 .. 383 of batch 0 and rows 0 .. 127 of batch 1, its window is batch stride - 129 rows (+ K): with 2^31 + 4096 elements that
    is 2^32 - 24,576 bytes -- the tile starts 64 KiB into batch 0, so the window still fits and the large tile runs across the jump;
    with 2^31 + 32768 it is 2^32 + 32,768 bytes and the dispatch must keep the 128 x 128 kernel (kind 0)."""
    _need_memory()
    K, N, B = 128, 256, 2
    bs = (1 << 31) + extra
    buf = torch.empty(bs + L * K, dtype=BF, device=DEV)
    try:
        a = torch.as_strided(buf, (B, L, K), (bs, K, 1))
        a.copy_(_randn((B, L, K), 21))
        w = _randn((N, K), 22, std=K ** -0.5)
        bias = _randn((N,), 23, std=0.1, dtype=torch.float32)
        a_small = a.contiguous()
        want = hip_lib.lib.osk_gemm_tile_choice(B * L, N, K)
        assert want in (1, 2) and hip_lib.gemm_tile_kind(a_small, w) == want
        kind = hip_lib.gemm_tile_kind(a, w)
        assert kind == (want if fits else 0)
        got = hip_lib.gemm(a, w, bias, torch.empty(B, L, N, dtype=BF, device=DEV))
        try:
            hip_lib.lib.osk_gemm_tile_override(kind)           # the contiguous copy on the same kernel
            assert hip_lib.gemm_tile_kind(a_small, w) == kind
            ref = hip_lib.gemm(a_small, w, bias, torch.empty(B, L, N, dtype=BF, device=DEV))
        finally:
            hip_lib.lib.osk_gemm_tile_override(-1)
        torch.cuda.synchronize()
        assert torch.equal(got, ref)
        v = _f64_rows(a_small.view(B * L, K), w, bias)
        bf16_ulp_close(got.view(B * L, N).float().cpu(), v.float().bfloat16().float(), rel=2 ** -7, abs_=2e-3)
    finally:
        del buf
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ case 3: W past 4 GiB
@pytest.mark.parametrize("N", [512, 520])
def test_w_past_4gib(hip_lib, N):
    """weight rows 2^22 + 64 elements apart, M = 512.  N = 512: the image is 512 x 8 MiB + 64 KiB, its last row STARTS 8 MiB below
    4 GiB; N = 520 (a ragged last column tile) reads rows that start past it.  By the estimate (256 x 128 tiles at this size) and on
    the 256 x 256 tiles."""
    _need_memory()
    K, M = 128, 512
    wrs = (1 << 22) + 64
    buf = torch.empty((N - 1) * wrs + K, dtype=BF, device=DEV)
    try:
        w = torch.as_strided(buf, (N, K), (wrs, 1))
        w.copy_(_randn((N, K), 31, std=K ** -0.5))
        assert N * wrs * 2 > GIB4 and (N == 512 or (N - 1) * wrs * 2 > GIB4)
        a = _randn((1, M, K), 32)
        bias = _randn((N,), 33, std=0.1, dtype=torch.float32)
        w_small = w.contiguous()
        want = hip_lib.lib.osk_gemm_tile_choice(M, N, K)
        assert want in (1, 2)
        try:
            for forced in (-1, 2):
                hip_lib.lib.osk_gemm_tile_override(forced)
                kind = hip_lib.gemm_tile_kind(a, w)
                assert kind == hip_lib.gemm_tile_kind(a, w_small) == (want if forced < 0 else forced)
                got = hip_lib.gemm(a, w, bias, torch.empty(1, M, N, dtype=BF, device=DEV))
                ref = hip_lib.gemm(a, w_small, bias, torch.empty(1, M, N, dtype=BF, device=DEV))
                torch.cuda.synchronize()
                assert torch.equal(got, ref), f"tile kind {kind}"
                v = _f64_rows(a[0], w_small, bias)
                bf16_ulp_close(got[0].float().cpu(), v.float().bfloat16().float(), rel=2 ** -7, abs_=2e-3)
        finally:
            hip_lib.lib.osk_gemm_tile_override(-1)
    finally:
        del buf
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ case 4: osk_gemm_group_bf16
def test_gemm_group_on_activations_past_4gib(hip_lib, y_buffer):
    """One plain task and one V^T task (head dim 128, H * hd = 256) whose activations are two "batches" of 1,024 rows of the y-shaped
    buffer -- its first and its last 1,024 rows, (M - 1024) * 21504 elements = 4.26 GB apart, the last of them past 4 GiB from the first
    -- by pointer offset.  The library used to
    decline the group (OSK_EUNSUPPORTED -> gemm_group() False).  The plain task equals osk_gemm_bf16 on the 256 x 256 tiles bit for bit;
    the V^T task equals osk_gemm_bf16 + osk_v_transpose_bf16 from a contiguous copy to the last-bit allowance include/osk.h states
    (the bias is added after the K loop), and the f64 product."""
    K, H, hd, L, B, N = 128, 2, 128, 1024, 2, 256
    bs = (M_Y - L) * YS
    assert ((B - 1) * bs + (L - 1) * YS + K) * 2 > GIB4 > bs * 2         # the second batch straddles the 4 GiB crossing
    x = torch.as_strided(y_buffer, (B, L, K), (bs, YS, 1), 6144)
    x.copy_(_randn((B, L, K), 41))
    wp, wv = _randn((N, K), 42, std=K ** -0.5), _randn((H * hd, K), 43, std=K ** -0.5)
    bp, bv = _randn((N,), 44, std=0.1, dtype=torch.float32), _randn((H * hd,), 45, std=0.3, dtype=torch.float32)
    out = torch.empty(B, L, N, dtype=BF, device=DEV)
    vt = torch.full((B, H, hd, L), 7.0, dtype=BF, device=DEV)
    assert hip_lib.gemm_group([dict(a=x, w=wp, bias=bp, out=out), dict(x=x, w=wv, bias=bv, vt=vt, vt_pos=0, hd=hd)]), \
        "osk_gemm_group_bf16 declined activations past 4 GiB (OSK_EUNSUPPORTED)"
    x_small = x.contiguous()
    try:
        hip_lib.lib.osk_gemm_tile_override(2)                  # the group runs on the 256 x 256 tiles whatever the estimate says
        ref = hip_lib.gemm(x_small, wp, bp, torch.empty(B, L, N, dtype=BF, device=DEV))
        v = hip_lib.gemm(x_small, wv, bv, torch.empty(B, L, H * hd, dtype=BF, device=DEV))
    finally:
        hip_lib.lib.osk_gemm_tile_override(-1)
    ref_vt = torch.zeros(B, H, hd, L, dtype=BF, device=DEV)
    hip_lib.v_transpose(v, ref_vt, H, hd)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    bf16_ulp_close(vt.float().cpu(), ref_vt.float().cpu(), rel=2 ** -7, abs_=2e-3)
    from tests import cpu_ops
    key = cpu_ops.pos2key(hd, L)
    v64 = x_small.double().cpu() @ wv.double().cpu().T + bv.double().cpu()
    ref64 = v64[:, key].reshape(B, L, H, hd).permute(0, 2, 3, 1)
    bf16_ulp_close(vt.float().cpu(), ref64.float().bfloat16().float(), rel=2 ** -7, abs_=2e-3)


# ------------------------------------------------------------------------------------------------ case 5: osk_gemm_fp8
def test_gemm_fp8_on_activations_past_4gib(hip_lib):
    """A8: M = 66,048 rows 65,536 bytes apart (4.33 GB), K = 256 (two K steps), N = 256.  The entry used to return OSK_EUNSUPPORTED
    (the binding raises on any non-zero status); now it equals the run from the contiguous image bit for bit and the f64 product of
    the dequantised operands on the sampled rows."""
    _need_memory()
    M, K, N, rs = 66048, 256, 256, 65536
    assert (M - 1) * rs > GIB4
    buf = torch.empty((M - 1) * rs + K, dtype=torch.uint8, device=DEV)
    try:
        a8_small, sa = hip_lib.quantize_rows_fp8(_randn((1, M, K), 51))
        w8, sw = hip_lib.quantize_rows_fp8(_randn((N, K), 52, std=K ** -0.5))
        a8 = torch.as_strided(buf, (M, K), (rs, 1))
        a8.copy_(a8_small)
        bias = _randn((N,), 53, std=0.1, dtype=torch.float32)
        got = hip_lib.gemm_fp8(a8, sa, w8, sw, bias, torch.empty(1, M, N, dtype=BF, device=DEV))
        ref = hip_lib.gemm_fp8(a8_small, sa, w8, sw, bias, torch.empty(1, M, N, dtype=BF, device=DEV))
        torch.cuda.synchronize()
        assert torch.equal(got, ref)
        rows = _sample_rows(M)
        deq = lambda q8, s: q8.cpu().view(F8).double() * s.cpu().double()[:, None]
        v = deq(a8_small[rows], sa[rows]) @ deq(w8, sw).T + bias.double().cpu()
        bf16_ulp_close(got[0, rows].float().cpu(), v.float().bfloat16().float(), rel=2 ** -7, abs_=2e-3)
        # the host layer's own rule follows the library: an fp8 image past 4 GiB qualifies
        assert hip_lib.gemm_fp8_supported(3 * 230912, 3072, 15360) and not hip_lib.gemm_fp8_supported(255, 3072, 15360)
    finally:
        del buf
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ case 7: one 11B single-stream block
def test_11b_single_block_with_y_past_4gib(hip_lib):
    """An 11B-width single-stream block (hidden 3072, 24 heads of 128, random weights) at B = 1, L = 100,096: its fused buffer y is
    4.3 GB.  Once as shipped -- linear1 in its group form with the V^T task and linear2 on the 256 x 256 tiles -- and once with every
    GEMM forced to the 128 x 128 kernel, which took this size before.  The V^T group must still be on after the shipped run.

    Tolerance: the rule tests/test_gpu_baseline_geometry.py applies to one block against its oracle (tests/util.assert_parity),
    e <= max(1.5 e_ref, 2^-8) and max|d| <= max(4 a_ref, 2^-8 max|out|), with the 128 x 128 run in the oracle's place.  No
    reference-precision comparator can be run at this length, so e_ref is dropped (the floor 2^-8 alone) and a_ref is replaced by
    what the output format alone guarantees of any bf16 comparator: half a bf16 step of the largest outputs, a_ref >= 2^-9 * 2^e for
    max|out| in [2^e, 2^(e+1)) -- i.e. 4 a_ref = two bf16 steps of the largest output."""
    _need_memory(14)
    from open_sora_amd import mmdit

    D, H, hd, L = 3072, 24, 128, M_Y
    torch.manual_seed(7)
    with torch.device(DEV):
        blk = mmdit.SingleStreamBlock(D, H, mlp_ratio=4.0).to(BF)
    x = _randn((1, L, D), 71)
    vec = _randn((1, D), 72)
    pos = torch.arange(L, dtype=torch.float32)
    ids = torch.stack((torch.zeros(L), torch.floor(pos / 389), pos % 389), -1)[None]
    from oracle import mmdit_oracle as O
    from open_sora_amd import configs as pcfg
    cfg = pcfg.MMDIT["11B"]
    ang = O.rope_angles(ids, cfg["axes_dim"], cfg["theta"])
    c, s = torch.cos(ang), torch.sin(ang)
    pe = torch.stack([c, -s, s, c], dim=-1).reshape(*ang.shape, 2, 2).float().unsqueeze(1).to(DEV)
    R = blk.mlp_hidden_dim
    try:
        with torch.inference_mode():
            shipped = blk(x, vec, pe)
            torch.cuda.synchronize()
            ws = mmdit._workspace(mmdit._PROC_POOL, 1, 0, L, D, R, H, hd, x.device)
            assert ws.y.numel() * 2 > GIB4
            assert ws.vt_group, "the library declined linear1's group (plain task + V^T task) on the > 4 GiB buffer"
            y_view = ws.y_single(D, R)
            assert hip_lib.gemm_tile_kind(y_view[:, :, 2 * D:], blk.linear2.weight) == 2       # linear2 reads y
            assert hip_lib.gemm_tile_kind(ws.xm, blk.linear1.weight) == 2
            try:
                hip_lib.lib.osk_gemm_tile_override(0)
                ws.vt_group = False                                                      # the group has no 128 x 128 form: the single calls
                small_tiles = blk(x, vec, pe)
                torch.cuda.synchronize()
            finally:
                hip_lib.lib.osk_gemm_tile_override(-1)
                ws.vt_group = True
        assert torch.isfinite(shipped).all()
        d = (shipped.float() - small_tiles.float())
        e = float(torch.linalg.vector_norm(d, dtype=torch.float64) / torch.linalg.vector_norm(small_tiles, dtype=torch.float64))
        a, top = float(d.abs().max()), float(small_tiles.float().abs().max())
        import math
        step = 2.0 ** (math.floor(math.log2(top)) - 7)
        print(f"11B single block, L = {L}: 256 x 256 tiles vs 128 x 128 tiles: relL2 {e:.3e}, max|d| {a:.3e} (max|out| {top:.3e}, bf16 step {step:.3e})")
        assert e <= 2.0 ** -8, e
        assert a <= max(2 * step, 2.0 ** -8 * top), (a, step, top)
    finally:
        if hasattr(mmdit._PROC_POOL, "_osk_ws_cache"):
            del mmdit._PROC_POOL._osk_ws_cache
        torch.cuda.empty_cache()
