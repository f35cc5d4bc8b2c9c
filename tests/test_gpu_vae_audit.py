"""GPU audit of the causal 3-D VAE convolution kernels (csrc/conv3d.hip, csrc/conv3d_256.hip): every host-side dispatch class at its
edges, every output element against a plain f64 reference of  upsample -> replicate / causal pad -> conv -> + bias (+ res).

Cases, seeded operands, references and the acceptance checks live in tests/vae_kernel_cases.py; tests/test_vae_kernel_refs.py runs the
same checks on an f32 control and on mutants of it without a GPU, which is where the tolerance is settled.  Each case here:
asserts the kernel class the call reaches (osk_causal_conv3d_kernel_class: the selection code the launch switches on); places x, w,
bias, res, out, gn_sums and the GroupNorm table inside sentinel-filled allocations with guard bands before and after; runs the kernel;
compares EVERY element; requires the guards and every byte of the inputs to come back bit for bit; repeats on tightly packed operands
and requires bit-equal output; runs the in-place-capable and multi-tile cases three times in all and requires bit-equal results; and,
where the case carries gn_G, runs the fused-statistics entry point too (fused, the same output bits, sums within 2e-5 of their
magnitude of the f64 statistics of that output).  The measured err / tol is printed before it is asserted (pytest -s).

What reaches which kernel class (ids as pytest prints them):
  tile128        conv3d_kernel<false>        [legacy00 01 08 09] (the CONV_CASES of test_gpu_vae.py), [exact_tile128]
  tile128_bigc   conv3d_kernel<true>         [legacy02 03 05 06 07 10 11 12], [exact_tile128_bigc] (strided)
  fewout         conv_fewout_kernel<1..4>    [fewout1] [fewout2] (NC 1, 2; Ho = 5: partial last row group), [legacy19 20] (NC 3, 4), [exact_fewout]
  conv256x4      conv256x_kernel<4>          generic epilogue [gen_x4_co136] [gen_x4_co200] [gen_x4_co200_res] [gen_x4_out8] [gen_x4_res8];
                                             [x4_B2_stats]; [multi_x4]; [legacy04 14 15]; [exact_x4]
  conv256x8      conv256x_kernel<8>          generic epilogue [gen_x8_co264] [gen_x8_co328_res] [gen_x8_out8] [gen_x8_res8]; [x8_B2_stats];
                                             [multi_x8]; [legacy13 16 17]; [exact_x8]
  convsw4        convsw_kernel<4>            odd block count [sw4_co160]; generic epilogue [gen_sw4_co136]; [sw4_B2_stats]; [multi_sw4];
                                             [legacy24 25]; [exact_sw4]
  convsw8        convsw_kernel<8>            odd block count [sw8_co288]; [multi_sw8]; [legacy22 23]; [exact_sw8]
  convsw4_up     convsw_kernel<4, UP>        [sw4up_co160] [sw4up_T1] [sw4up_B2]; [legacy28]; [exact_sw4_up]
  convsw8_up     convsw_kernel<8, UP>        [sw8up_co288] [sw8up_T1] [sw8up_hw] [sw8up_B2]; [multi_sw8up]; [legacy18 27 29]; [exact_sw8_up]
  convsw8_gn     convsw_kernel<8, false, GN> [sw8gn_co288]; [multi_sw8gn]; [exact_sw8_gn]
  convsw2        convsw2_kernel<false>       [sw2_B2_T3] [sw2_B2_T5]; generic epilogue [gen_sw2_out8]; [multi_sw2]; [legacy21 26]; [exact_sw2]
  convsw2_gn     convsw2_kernel<true>        [sw2gn_B2_T3]; [exact_sw2_gn]
The multi_* cases take their extent from the device's CU count: more tiles than CUs and a partial last round on any part.

Further down, in the same style: the GroupNorm kernels of csrc/groupnorm.hip (test_groupnorm_every_class_edge: cpg 1 .. 16 x S 1, 1023,
1025, 2500; test_groupnorm_stats_with_a_large_mean) and csrc/attention_hd512.hip (test_attention_hd512_selector_rows: [3x64] [2x37]
[2x37_nomask] [4x1024_split], the last through the key-split launch).
"""
import functools

import pytest
import torch

from tests import vae_kernel_cases as VC
from tests.test_gpu_row_kernels import _SENTINEL, bits, sentinel

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
GUARD = 64          # elements: 128 bytes of bf16, a multiple of 16 bytes for every dtype used


def place(t: torch.Tensor, off: int = 0):
    """t inside a sentinel-filled flat allocation, GUARD (+ off) elements in front and GUARD behind -> (flat, view, off)"""
    n = t.numel()
    flat = sentinel((GUARD + off + n + GUARD,), t.dtype)
    view = flat[GUARD + off: GUARD + off + n].view(t.shape)
    view.copy_(t)
    return flat, view, off


def assert_guards(flat: torch.Tensor, n: int, off: int, what: str) -> None:
    want = _SENTINEL[flat.element_size()]
    b = bits(flat)
    assert bool((b[: GUARD + off] == want).all()), f"{what}: wrote in front of the buffer"
    assert bool((b[GUARD + off + n:] == want).all()), f"{what}: wrote behind the buffer"


def place_sums(B: int, G: int):
    """zeroed f64 [B, G, 2] between guard bands (the sentinel is held as 32-bit words)"""
    n = B * G * 2
    flat = sentinel((2 * (n + 2 * GUARD),), torch.float32)
    sums = flat.view(torch.float64)[GUARD: GUARD + n].view(B, G, 2)
    sums.zero_()
    return flat, sums


def assert_sums_guards(flat: torch.Tensor, n: int) -> None:
    b = bits(flat)
    assert bool((b[: 2 * GUARD] == _SENTINEL[4]).all()) and bool((b[2 * (GUARD + n):] == _SENTINEL[4]).all()), "gn_sums: wrote outside"


@functools.lru_cache(maxsize=None)
def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _call(hip_lib, c, x, w, bias, out, res, table, sums=None):
    if c.gn_in:
        ran, fused = hip_lib.causal_conv3d_gn_in(x, table, w, bias, out, c.k, res=res, gn_sums=sums)
        assert ran, "the folded-GroupNorm entry point declined the shape"
        return fused
    if sums is None:
        hip_lib.causal_conv3d(x, w, bias, out, c.k, c.stride, c.up, res)
        return False
    return hip_lib.causal_conv3d(x, w, bias, out, c.k, c.stride, c.up, res, gn_sums=sums)[1]


@pytest.mark.parametrize("cid", [c.id for c in VC.CONV_CASES])
def test_conv_every_class_and_edge(hip_lib, cid):
    o = VC.operands(cid, _cus())
    c = o["case"]
    oshape = (o["B"], o["To"], o["Ho"], o["Wo"], c.Cout)
    n_out = o["B"] * o["To"] * o["Ho"] * o["Wo"] * c.Cout
    if c.multi:
        ntiles = VC.multi_extent(c, _cus())[4]
        print(f"{cid}: {ntiles} tiles on {_cus()} CUs")
    assert hip_lib.conv_kernel_class(**VC.report_args(o)) == (c.cls, False)

    ins = dict(x=place(o["x"]), w=place(o["w"]), bias=place(o["bias"]))
    if o["res"] is not None:
        ins["res"] = place(o["res"], c.res_off)
    if c.gn_in:
        ins["table"] = place(o["table"])
    v = {k: t[1] for k, t in ins.items()}
    assert (v["res"].data_ptr() % 16 == 8) == bool(c.res_off) if c.res else True

    def run(sums=None):
        flat = sentinel((GUARD + c.out_off + n_out + GUARD,), BF)
        out = flat[GUARD + c.out_off: GUARD + c.out_off + n_out].view(oshape)
        assert (out.data_ptr() % 16 == 8) == bool(c.out_off)
        fused = _call(hip_lib, c, v["x"], v["w"], v["bias"], out, v.get("res"), v.get("table"), sums)
        torch.cuda.synchronize()
        assert_guards(flat, n_out, c.out_off, "out")
        return out, fused

    out, _ = run()
    for k, (flat, view, off) in ins.items():
        assert_guards(flat, view.numel(), off, k)
        assert torch.equal(bits(view).cpu(), bits(o[k])), f"{k} was modified"
    ref = VC.reference(o, DEV) if c.multi else _cpu_ref(cid)
    slack = VC.gn_in_slack(o, DEV if c.multi else "cpu") if c.gn_in and not c.structured else None
    VC.check_conv(out.reshape(-1, c.Cout).cpu(), ref, o, slack=slack)

    # tightly packed, 16-byte aligned operands: the same bits (for the out_off / res_off cases: generic against fast epilogue)
    packed = {k: o[k].to(DEV).contiguous() for k in ins}
    out_p = torch.full(oshape, float("nan"), dtype=BF, device=DEV)
    _call(hip_lib, c, packed["x"], packed["w"], packed["bias"], out_p, packed.get("res"), packed.get("table"))
    torch.cuda.synchronize()
    assert torch.equal(bits(out_p), bits(out)), "guard-banded and packed operands give different bits"
    if c.repeat or c.multi:
        for _ in range(2):
            assert torch.equal(bits(run()[0]), bits(out)), "two runs on the same input differ"
    if c.gn_G:
        assert hip_lib.conv_kernel_class(**VC.report_args(o, stats=True)) == (c.cls, True)
        sflat, sums = place_sums(o["B"], c.gn_G)
        out_s, fused = run(sums)
        assert fused, "the fused-statistics entry point declined the shape"
        assert_sums_guards(sflat, sums.numel())
        assert torch.equal(bits(out_s), bits(out)), "the fused-statistics epilogue changes the output"
        VC.check_stats(sums, out, o["B"], c.gn_G, cid)


@functools.lru_cache(maxsize=None)
def _cpu_ref(cid):
    return VC.reference(VC.operands(cid, _cus()))


def test_fused_statistics_are_declined_with_nothing_launched(hip_lib):
    """Cout % 32 != 0, and a residual that is only 8-byte aligned (the epilogue's generic path carries no statistics): the report says
    unsupported, the entry point returns the same status, out and gn_sums keep their sentinels"""
    for cid, G in (("gen_x4_co136", 17), ("gen_x8_res8", 32)):
        o = VC.operands(cid, _cus())
        c = o["case"]
        assert hip_lib.conv_kernel_class(**dict(VC.report_args(o), gn_groups=G)) == -2
        x, w, bias = o["x"].to(DEV), o["w"].to(DEV), o["bias"].to(DEV)
        res = None if o["res"] is None else place(o["res"], c.res_off)[1]
        n_out = o["To"] * o["Ho"] * o["Wo"] * c.Cout
        flat = sentinel((n_out + 2 * GUARD,), BF)
        out = flat[GUARD: GUARD + n_out]
        sflat, sums = place_sums(1, G)
        rc = hip_lib.lib.osk_causal_conv3d_gn_ndhwc_bf16(x.data_ptr(), 1, o["T"], o["H"], o["W"], c.Cin, w.data_ptr(), w.stride(0),
                                                         bias.data_ptr(), c.Cout, 3, 1, 1, 1, 0, 0, None if res is None else res.data_ptr(),
                                                         out.data_ptr(), o["To"], o["Ho"], o["Wo"], sums.data_ptr(), G, hip_lib._stream())
        torch.cuda.synchronize()
        assert rc == -2
        assert bool((bits(flat) == _SENTINEL[2]).all()) and float(sums.abs().sum()) == 0.0
        assert_sums_guards(sflat, sums.numel())


# ----------------------------------------------------------------------------- GroupNorm kernels (csrc/groupnorm.hip)
def test_groupnorm_every_class_edge(hip_lib):
    """gn_stats, gn_table and gn_apply at cpg 1 .. 16 and S of 1, 1023, 1025, 2500 (VC.GN_CASES), operands and outputs between guard
    bands.  stats: f64 sums within 2e-5 of their magnitude.  table: the f64 a, d within the f32 roundings of their expressions.
    apply (fed the exact f64 sums, with and without SiLU): every element within one bf16 step per rounding point of the f64
    statement; the pooled share of elements that differ at all is printed and capped at twice the f32 control's."""
    nd = tot = 0
    for C, G, S in VC.GN_CASES:
        c = VC.gn_case(C, G, S)
        xf, x, _ = place(c["x"])
        sflat, sums = place_sums(VC.GN_B, G)
        hip_lib.groupnorm_stats(x, G, sums)
        torch.cuda.synchronize()
        assert_sums_guards(sflat, sums.numel())
        VC.check_gn_stats(sums, c)
        exact = c["sums"].to(DEV)
        tflat, table, _ = place(torch.zeros(VC.GN_B, C // 8, 16))
        hip_lib.groupnorm_table(exact, c["gamma"].to(DEV), c["beta"].to(DEV), table, S, G, VC.GN_EPS)
        torch.cuda.synchronize()
        assert_guards(tflat, table.numel(), 0, "table")
        VC.check_gn_table(table, c)
        for silu in (False, True):
            oflat, out, _ = place(torch.zeros_like(c["x"]))
            bits(out).fill_(_SENTINEL[2])
            hip_lib.groupnorm_apply(x, exact, c["gamma"].to(DEV), c["beta"].to(DEV), out, G, VC.GN_EPS, silu)
            torch.cuda.synchronize()
            assert_guards(oflat, out.numel(), 0, "out")
            d, n = VC.check_gn_apply(out, c, silu)
            nd, tot = nd + d, tot + n
        assert_guards(xf, x.numel(), 0, "x")
        assert torch.equal(bits(x).cpu(), bits(c["x"]))
    print(f"gn_apply: {nd} of {tot} elements differ from the f64 statement ({nd / tot:.3e}; cap {VC.GN_SHARE_CAP:.3e})")
    assert nd / tot <= VC.GN_SHARE_CAP


def test_groupnorm_stats_with_a_large_mean(hip_lib):
    """|mean| rstd at twice the largest of the full-size config-3 encode and decode: var = E[x^2] - mean^2 cancels, the kernel keeps f32
    per-thread partials -- the rstd from its sums must agree with the f64 two-pass rstd to 2^-10"""
    c = VC.gn_case(*VC.GN_BIG_CASE, VC.GN_BIG_RATIO)
    sums = torch.empty(VC.GN_B, c["G"], 2, dtype=torch.float64, device=DEV)
    hip_lib.groupnorm_stats(c["x"].to(DEV), c["G"], sums)
    torch.cuda.synchronize()
    err = VC.gn_rstd_error(sums, c)
    print(f"large-mean stats: |mean| rstd {float((c['mean'].abs() * c['rstd']).max()):.2f}, rstd error {err:.3e} (allowed {VC.GN_RSTD_REL:.3e})")
    assert err <= VC.GN_RSTD_REL


# ----------------------------------------------------------------------------- attention_hd512
@pytest.mark.parametrize("name", [c[0] for c in VC.HD_CASES])
def test_attention_hd512_selector_rows(hip_lib, name):
    """osk_attention_hd512_fwd_ws_bf16 against f64 with the derived per-element tolerance (VC.hd_reference; no flat 2^-7): random
    rows plus selector rows whose weight sits on key 0, 31, 32, S - 1, the last key of the query's own frame and the first key of
    the next frame (masked: that key's V must be absent).  q, k column views of one guard-banded buffer, V^T and out between guard
    bands; two runs bit-equal; the key-split launch (workspace) for S >= 4096."""
    c = VC.hd_case(name)
    S, C = c["S"], VC.HD_C
    Sp = (S + 63) // 64 * 64
    qkf, qk, _ = place(torch.cat((c["q"], c["k"]), 2))
    q, k = qk[:, :, :C], qk[:, :, C:]
    vt0 = torch.zeros(1, C, Sp, dtype=BF)
    vt0[:, :, :S] = c["v"].transpose(1, 2)
    vf, vt, _ = place(vt0)
    bias = c["bias"].to(DEV)
    ws = hip_lib.attention_hd512_workspace(1, S, DEV) if c["split"] else None
    rt = VC.hd_reference(c)
    outs = []
    for _ in range(2):
        of, out, _ = place(torch.zeros(1, S, C, dtype=BF))
        bits(out).fill_(_SENTINEL[2])
        hip_lib.attention_hd512(q, k, vt, bias, out, c["hw"] if c["masked"] else 0, VC.HD_SCALE, workspace=ws)
        torch.cuda.synchronize()
        assert_guards(of, out.numel(), 0, "out")
        outs.append(out)
    VC.check_hd(outs[0], c, rt)
    assert torch.equal(bits(outs[0]), bits(outs[1])), "two runs differ"
    assert_guards(qkf, qk.numel(), 0, "q, k")
    assert_guards(vf, vt.numel(), 0, "V^T")
    assert torch.equal(bits(vt).cpu(), bits(vt0))
