"""GPU audit of the hand-scheduled flash-attention family against f64, row by row: every case of tests/attention_cases.py (diffuse,
selector and special rows in one call; operands inside guard-banded allocations) with the derived per-element tolerances of
tests/cpu_ops_attn_f64.py, and osk_v_transpose_fp8 bit for bit.  tests/test_attention_refs.py shows on the CPU that the tolerances
admit a correct kernel and reject five single-key defects on these same operands; profiles/attn_audit.md records the ratios and the
six device mutants this file rejects."""
import pytest
import torch

from tests import attention_cases as A
from tests import cpu_ops
from tests import cpu_ops_attn_f64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _heads_out(case, out):
    return out.float().cpu().reshape(case.B, case.Lq, case.H, case.hd).permute(0, 2, 1, 3)


@pytest.mark.parametrize("name", [c.name for c in A.CASES])
def test_attention_audit(hip_lib, name):
    c, ops, ref = A.BY_NAME[name], A.operands(name), A.reference(name)
    try:
        if c.wide:   # small shapes never fill the chip with 512-row units: the documented tool switch selects the layout, the library
            assert hip_lib.lib.osk_attention_rows_override(512) == 0   # still decides whether it is legal (launch shape asserted below)
        L = A.layout(hip_lib, c, ops, DEV)
        ws_bytes = 0 if L["ws"] is None else L["ws"].numel()
        body, parts, rows = A.dispatch(hip_lib, c, ops, ws_bytes)
        assert (body, parts, rows) == ("FAST" if c.body == "pair" else c.body, c.split, c.rows), (body, parts, rows)
        if c.api == "auto":   # the device's own norms put (batch, head) pairs on both sides of the FAST limit: both twins work
            b = (L["qn2"] * L["kn2"][torch.arange(c.B, device=DEV) % c.nb]).sqrt() * 1.004
            assert b.min().item() <= 56.0 < b.max().item(), b
        before = A.snapshot(L)
        A.call(hip_lib, c, ops, L)
        torch.cuda.synchronize()
        bad = A.disturbed(L, before)
        Lp = A.layout(hip_lib, c, ops, DEV, packed=True)
        A.call(hip_lib, c, ops, Lp)
        torch.cuda.synchronize()
    finally:
        if c.wide:
            hip_lib.lib.osk_attention_rows_override(0)
    out, lse = _heads_out(c, L["out"]), L["lse"].cpu()
    r_out, r_lse = R.ratios(out, lse, ref)
    print(f"audit {c.klass:15s} {name:40s} err/tol {r_out:.3f}  dlse/tol {r_lse:.3f}")
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()
    assert r_out <= 1.0, r_out
    assert r_lse <= 1.0, r_lse
    assert not bad, f"bytes outside the call's outputs changed in allocation(s) {bad}"
    assert torch.equal(L["out"].contiguous().view(torch.int16), Lp["out"].view(torch.int16)), "guarded and packed operands differ"
    assert torch.equal(L["lse"].contiguous().view(torch.int32), Lp["lse"].contiguous().view(torch.int32))


def vt8_pos2key() -> torch.Tensor:
    """byte p of a 64-key tile row of vt8 holds key 32 t2 + 8 j + 4 hi + i, with hi = p / 32, t2 = p / 16 % 2, j = p / 4 % 4,
    i = p % 4: the order in which a lane of the score accumulators holds its 32 P values (csrc/attention_fwd.hip)"""
    p = torch.arange(64)
    return 32 * ((p >> 4) & 1) + 8 * ((p >> 2) & 3) + 4 * (p >> 5) + (p & 3)


def _fix0(t):
    return torch.where(t == 0x80, torch.zeros_like(t), t)


@pytest.mark.parametrize("hd", [72, 128])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 150])
def test_v_transpose_fp8_bit_exact(hip_lib, hd, L):
    B, H = 2, 2
    D = H * hd
    g = torch.Generator().manual_seed(500 + L)
    y = (torch.randn(B, L + 3, 3 * D, generator=g) * 1.3).to(BF).to(DEV)
    v = y[:, 3:, 2 * D:]                            # strided view inside a fused projection buffer
    v[0, :, :hd] = 0                                 # an all-zero head: scale 1, bytes 0
    v[B - 1, L // 2, D - 5] = 200.0                  # an outlier that owns its head's scale
    s = hip_lib.v_scale_fp8(v, H, hd)
    assert torch.equal(s.cpu(), cpu_ops.v_scale_fp8(v.cpu(), H, hd))
    rp, Lp = hip_lib.vt8_rows(hd), (L + 63) // 64 * 64
    n = B * H * rp * Lp
    buf = torch.full((n + 512,), 0xAA, dtype=torch.uint8, device=DEV)   # vt8 is one contiguous tensor: the guards lie around it
    vt8 = buf[256:256 + n].view(B, H, rp, Lp)
    hip_lib.v_transpose_fp8(v, s, vt8, H, hd)
    ref = torch.zeros(B, H, rp, Lp, dtype=torch.uint8)
    cpu_ops.v_transpose_fp8(v.cpu(), s.cpu(), ref, H, hd)                # natural key order; the ones row and the zero rows included
    col = (torch.arange(Lp) // 64 * 64) + vt8_pos2key().repeat(Lp // 64)
    assert torch.equal(_fix0(vt8.cpu()), _fix0(ref[..., col]))
    assert (buf[:256] == 0xAA).all() and (buf[256 + n:] == 0xAA).all()
