"""GPU: osk_attention_merge_bf16 (csrc/attention_merge.hip) against the f64 statement of the merge on the SAME bf16 partials and
f32 lse values (tests/cpu_ops_sp_chunked.py::attention_merge_f64).

Bound, every element, none left out:  |out - exact| <= 2^-8 |exact| + 2^-20 sum_s wbar_s |part_s|  (wbar = the normalised weights).
The first term is the ONE bf16 rounding of the f32 sum (half an ulp is 2^-9 of the value; 2^-8 as everywhere in this suite); the
second covers the f32 arithmetic in front of it: a weight carries the error of expf (<= 2 ulp) and of the subtraction in its
argument, the normalisation one division and a sum of <= 8 terms, the accumulation one fma per part -- under 16 ulp of f32 (2^-20)
of the magnitude sum_s wbar_s |part_s| the terms have.  lse_out: |d| <= 2^-19 + 2^-23 |lse| (the relative error of the weight
sum in [1, 8] through logf, plus the rounding of m + log)."""
import pytest
import torch

from tests.cpu_ops_sp_chunked import attention_merge_f64

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda:0"
NEG_INF = float("-inf")
KINDS = ("random", "equal", "ahead60", "one_inf", "all_inf")


def _lse(kind, S, B, H, L, g):
    lse = torch.randn(S, B, H, L, generator=g) * 2.0 + 5.0
    if kind == "equal":
        lse = lse[:1].expand(S, B, H, L).contiguous()
    elif kind == "ahead60":                        # the other weights underflow against the leader (exp(-60) ~ 9e-27)
        lse[S // 2] += 60.0
    elif kind == "one_inf":                        # (S = 1: the only part, i.e. the all-empty case)
        lse[S - 1] = NEG_INF
        lse[0, :, :, ::3] = NEG_INF if S > 2 else lse[0, :, :, ::3]      # two empty parts in some rows
    elif kind == "all_inf":
        lse[:, :, :, ::2] = NEG_INF                # every part empty in the even rows, ordinary odd rows beside them
    return lse


def _run_case(hip_lib, S, B, H, L, hd, kind, strided, with_lse_out, seed):
    g = torch.Generator().manual_seed(seed)
    D = H * hd
    parts_c = (torch.randn(S, B, L, D, generator=g) * 1.5).to(BF)
    lse_c = _lse(kind, S, B, H, L, g)
    exact, lse_exact, mag = attention_merge_f64(parts_c, lse_c)
    if strided:   # a strided part axis (every other slot of a [S, 2, ...] buffer) and output rows wider than D, sentinels around
        pbuf = torch.full((S, 2, B, L, D), 7.0, dtype=BF, device=DEV)
        pbuf[:, 0] = parts_c.to(DEV)
        parts = pbuf[:, 0]
        obuf = torch.full((B, L, D + 64), -3.0, dtype=BF, device=DEV)
        out = obuf[:, :, 32:32 + D]
        assert parts.stride(0) == 2 * B * L * D and out.stride(1) == D + 64
    else:
        parts = parts_c.to(DEV)
        obuf = torch.full((B, L, D), -3.0, dtype=BF, device=DEV)
        out = obuf
    lse = lse_c.to(DEV)
    lo = torch.full((B, H, L), 123.0, device=DEV) if with_lse_out else None
    hip_lib.attention_merge(parts, lse, out, H, hd, lse_out=lo)
    torch.cuda.synchronize()
    got = out.cpu().double()
    assert torch.isfinite(got).all(), f"non-finite output ({kind})"
    err, tol = (got - exact).abs(), 2.0 ** -8 * exact.abs() + 2.0 ** -20 * mag
    worst = float((err / tol.clamp_min(1e-300)).max()) if bool((tol > 0).any()) else 0.0
    assert bool((err <= tol).all()), (kind, S, B, H, L, hd, strided, worst, float(err.max()))
    empty = torch.isinf(lse_exact)                                          # [B, H, L]: every part empty
    if bool(empty.any()):
        rows = empty.permute(0, 2, 1).unsqueeze(-1).expand(B, L, H, hd).reshape(B, L, D)
        assert bool((got[rows] == 0).all()), "an all-empty (row, head) is not zero"
    if strided:
        ob = obuf.cpu().float()
        assert bool((ob[:, :, :32] == -3.0).all()) and bool((ob[:, :, 32 + D:] == -3.0).all()), "wrote outside the output columns"
    if with_lse_out:
        lg = lo.cpu().double()
        assert torch.equal(torch.isinf(lg) & (lg < 0), empty) and not torch.isnan(lg).any()
        fin = ~empty
        d = (lg[fin] - lse_exact[fin]).abs()
        assert bool((d <= 2.0 ** -19 + 2.0 ** -23 * lse_exact[fin].abs()).all()), (kind, float(d.max()))
    return worst


@pytest.mark.parametrize("hd", [64, 72, 128])
@pytest.mark.parametrize("H,B", [(1, 1), (3, 1), (1, 2), (3, 2)])
def test_merge_against_f64(hip_lib, hd, H, B):
    """every L in {1, 77, 130} (one row; rows that are no multiple of the block's 8; more than one block) x S in {1, 2, 3, 8} x
    every lse pattern, contiguous and strided, lse_out present and absent"""
    worst, seed = 0.0, 0
    for L in (1, 77, 130):
        for S in (1, 2, 3, 8):
            for i, kind in enumerate(KINDS):
                seed += 1
                strided = (i + S + L) % 2 == 0
                worst = max(worst, _run_case(hip_lib, S, B, H, L, hd, kind, strided, with_lse_out=(i + S) % 2 == 0, seed=seed))
    # both layouts and both lse_out settings for the ordinary pattern at the largest shape
    for strided in (False, True):
        for with_lse_out in (False, True):
            worst = max(worst, _run_case(hip_lib, 3, B, H, 130, hd, "random", strided, with_lse_out, seed=991))
    print(f"hd {hd} H {H} B {B}: largest err / bound {worst:.3f}")


def test_one_part_is_a_copy_and_a_merge_of_equal_parts_is_the_part(hip_lib):
    g = torch.Generator().manual_seed(1)
    B, L, H, hd = 2, 77, 3, 72
    p = (torch.randn(1, B, L, H * hd, generator=g)).to(BF).to(DEV)
    lse = torch.randn(1, B, H, L, generator=g).to(DEV)
    out, lo = torch.empty(B, L, H * hd, dtype=BF, device=DEV), torch.empty(B, H, L, device=DEV)
    hip_lib.attention_merge(p, lse, out, H, hd, lse_out=lo)
    assert torch.equal(out, p[0]) and torch.equal(lo, lse[0])
    p4, l4 = p.expand(4, B, L, H * hd).contiguous(), lse.expand(4, B, H, L).contiguous()
    hip_lib.attention_merge(p4, l4, out, H, hd, lse_out=lo)
    assert torch.equal(out, p[0])                                           # 4 x (0.25 x) : exact in f32
    assert float((lo - (lse[0] + 1.3862943611198906)).abs().max()) <= 2.0 ** -19 + 2.0 ** -23 * float(lse.abs().max() + 1.4)


def test_merge_is_graph_capturable(hip_lib):
    g = torch.Generator().manual_seed(2)
    S, B, L, H, hd = 3, 1, 130, 3, 128
    parts = torch.randn(S, B, L, H * hd, generator=g).to(BF).to(DEV)
    lse = torch.randn(S, B, H, L, generator=g).to(DEV)
    out, lo = torch.empty(B, L, H * hd, dtype=BF, device=DEV), torch.empty(B, H, L, device=DEV)
    call = lambda: hip_lib.attention_merge(parts, lse, out, H, hd, lse_out=lo)
    call()
    eager, eager_l = out.clone(), lo.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                   # side-stream warm-up, as torch's capture recipe asks
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        out.zero_()
        lo.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(lo, eager_l)
