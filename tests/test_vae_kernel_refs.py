"""CPU: the checks of tests/vae_kernel_cases.py admit f32 arithmetic and reject small defects, and the host-only kernel-class report
agrees with every case (no GPU).

The control is torch's f32 unfold-and-matmul on the case's own operands, rounded once to bf16: a correct kernel with another
summation order.  The multi-tile cases are evaluated on a sampled set of voxels here (extents for 256 CUs); the GPU audit
compares them in full."""
import functools

import pytest
import torch

from tests import vae_kernel_cases as VC

IDS = [c.id for c in VC.CONV_CASES]


def _vox(o):
    return VC.sample_voxels(o["B"] * o["To"] * o["Ho"] * o["Wo"]) if o["case"].multi else None


@functools.lru_cache(maxsize=None)
def _slack(cid):
    o = VC.operands(cid)
    return VC.gn_in_slack(o, "cpu", _vox(o)) if o["case"].gn_in and not o["case"].structured else None


@functools.lru_cache(maxsize=None)
def _ref(cid):
    o = VC.operands(cid)
    return VC.reference(o, "cpu", _vox(o))


@pytest.mark.parametrize("cid", IDS)
def test_control_passes_every_check(cid):
    """the f32 control passes.  CONV_A is four times the largest need measured (profiles/vae_audit.md); another BLAS sums in another
    order, so what is asserted here is half the bound, not the quarter that was measured"""
    o = VC.operands(cid)
    got = VC.control(o, _vox(o))
    VC.check_conv(got, _ref(cid), o, "control ", _slack(cid))
    if not o["case"].structured:
        need = VC.conv_need(got, _ref(cid))
        assert 2 * need <= VC.CONV_A, f"{cid}: the control needs {need:.3e} of max|y|: CONV_A must be four times the largest need"
    if o["case"].gn_G and not o["case"].multi:
        out = got.reshape(o["B"], -1, o["case"].Cout)
        exact, _ = VC.stats_exact(out, o["B"], o["case"].gn_G)
        VC.check_stats(exact.float().double(), out, o["B"], o["case"].gn_G, cid)     # f32-rounded sums pass the statistics rule


@pytest.mark.parametrize("mutant,cid", [(m, cid) for m, ids in VC.MUTANTS.items() for cid in ids])
def test_mutants_of_the_control_are_rejected(mutant, cid):
    o = VC.operands(cid)
    got = VC.control(o, _vox(o), mutant)
    assert not torch.equal(got.view(torch.int16), VC.control(o, _vox(o)).view(torch.int16)), "the mutant changes nothing in this case"
    with pytest.raises(AssertionError):
        VC.check_conv(got, _ref(cid), o, f"mutant {mutant} ", _slack(cid))


@pytest.mark.parametrize("cid", ["exact_x4", "exact_sw8", "exact_sw4_up", "exact_fewout"])
def test_structured_cases_detect_transposes(cid):
    """a swapped tap order, swapped 8-channel chunks and swapped (h, w) each change the exact integers"""
    o = VC.operands(cid)
    c = o["case"]
    K = 27 * c.Cin
    w3 = o["w"][:, :K].reshape(c.Cout, 3, 3, 3, c.Cin)
    for name, wm in (("taps (dh, dw) swapped", w3.transpose(2, 3)), ("taps reversed in time", w3.flip(1)),
                     ("8-channel chunks in reverse order", w3.reshape(c.Cout, 3, 3, 3, -1, 8).flip(4).reshape(w3.shape))):
        om = dict(o, w=torch.cat((wm.reshape(c.Cout, K), o["w"][:, K:]), 1))
        with pytest.raises(AssertionError):
            VC.check_conv(VC.control(om), _ref(cid), o, f"{name}: ")


def test_the_two_references_agree():
    """conv_unfold in f64 (the multi-tile reference) is F.conv3d in f64 (the small-case reference): upsample, stride, residual, GN-in"""
    for cid in ("legacy17_256to256", "legacy13_128to256", "sw2_B2_T5", "sw8gn_co288", "legacy09_32to32"):
        o = VC.operands(cid)
        c = o["case"]
        x = VC.gn_in_input(o["x"], o["table"]) if c.gn_in else o["x"]
        a = VC.conv_unfold(x, o["w"], o["bias"], o["res"], c)
        b = VC.conv_ref_small(o)
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()), cid


def test_every_class_is_reached_and_named_cases_exist():
    reached = {c.cls for c in VC.CONV_CASES}
    assert reached == set(VC.CLASSES)
    assert {c.cls for c in VC.CONV_CASES if c.structured} == set(VC.CLASSES)
    assert {c.cls for c in VC.CONV_CASES if c.multi} == {"conv256x4", "conv256x8", "convsw4", "convsw8", "convsw2", "convsw8_up", "convsw8_gn"}
    assert {c.cls for c in VC.CONV_CASES if c.gn_G} == set(VC.STATS_CLASSES)
    for cus in (256, 304, 64, 104):
        for c in VC.CONV_CASES:
            if c.multi:
                VC.multi_extent(c, cus)        # asserts ntiles > CUs and a partial last round


@pytest.mark.parametrize("cid", IDS)
def test_kernel_class_report_agrees_with_the_case(cid):
    """host only: the report is the selection code the launch switches on"""
    from open_sora_amd import _C

    assert _C.CONV_KERNEL_CLASSES == VC.CLASSES
    o = VC.operands(cid)
    c = o["case"]
    assert _C.conv_kernel_class(**VC.report_args(o)) == (c.cls, False)
    if c.gn_G:
        assert _C.conv_kernel_class(**VC.report_args(o, stats=True)) == (c.cls, True)
    if c.multi:       # the extents computed for other CU counts reach the same kernel
        for cus in (64, 304):
            B, T, H, W, _ = VC.multi_extent(c, cus)
            assert _C.conv_kernel_class(**dict(VC.report_args(o), B=B, T=T, H=H, W=W))[0] == c.cls


def test_kernel_class_report_refusals():
    """the statuses the entry points return, nothing launched: -2 = unsupported (the caller runs the plain path), -1 = invalid"""
    from open_sora_amd import _C

    k = _C.conv_kernel_class
    big = dict(B=1, T=2, H=10, W=13, Cin=128, ksize=3)
    assert k(Cout=136, gn_groups=17, **big) == -2                      # Cout % 32 != 0: declined, nothing launched
    assert k(Cout=160, gn_groups=32, **big) == -2                      # 5 channels per group
    assert k(Cout=256, gn_groups=8, **big) == -2                       # 32 channels per group
    assert k(Cout=256, gn_groups=32, **big) == ("conv256x8", True)
    assert k(Cout=256, gn_groups=32, out_align=8, **big) == -2         # the statistics ride in the 16-byte store path
    assert k(Cout=256, gn_groups=32, res_align=8, **big) == -2         # ... which a residual that is only 8-byte aligned turns off
    assert k(Cout=256, gn_groups=32, res_align=16, **big) == ("conv256x8", True)
    assert k(B=2, T=3, H=10, W=11, Cin=128, Cout=256, ksize=3, gn_groups=32) == -2      # a 256-voxel tile would straddle the items
    assert k(B=1, T=3, H=12, W=12, Cin=64, Cout=128, ksize=3, gn_groups=32) == -2       # small-tile kernel: no fused epilogue
    assert k(B=1, T=3, H=6, W=64, Cin=128, Cout=3, ksize=3, gn_groups=3) == -2          # few-output kernel: none either
    # folded GroupNorm: sliding-window kernels in plain geometry only
    sw = dict(B=1, H=16, W=16, ksize=3, gn_in=True)
    assert k(T=2, Cin=128, Cout=256, **sw) == ("convsw8_gn", False)
    assert k(T=2, Cin=128, Cout=128, **sw) == ("convsw2_gn", False)
    assert k(T=1, Cin=128, Cout=128, **sw) == -2                       # Cout == 128 needs frame pairs
    assert k(T=2, Cin=64, Cout=256, **sw) == -2                        # Cin % 128
    assert k(T=2, Cin=128, Cout=160, **sw) == -2                       # 128 < Cout < 256 has no GN form
    assert k(T=2, Cin=128, Cout=256, B=1, H=24, W=32, ksize=3, gn_in=True) == -2        # H is not whole bricks
    assert k(T=2, Cin=128, Cout=256, up=(False, True), **dict(sw, H=8, W=8)) == -2      # no GN form under the upsample
    assert k(T=2, Cin=128, Cout=256, gn_groups=32, **sw) == ("convsw8_gn", True)
    # argument checks shared with the entry points
    assert k(B=1, T=2, H=4, W=4, Cin=24, Cout=8, ksize=3) == -2        # Cin not 8 * 2^j
    assert k(B=1, T=2, H=4, W=4, Cin=32, Cout=8, ksize=3, w_row_stride=27 * 32) == -1   # rows not padded to whole K steps
    assert k(B=1, T=2, H=4, W=4, Cin=32, Cout=8, ksize=3, out_align=4) == -1            # out must be 8-byte aligned
    assert k(B=1, T=2, H=4, W=4, Cin=32, Cout=8, ksize=3, res_align=4) == -1
    assert k(B=1, T=2, H=4, W=4, Cin=32, Cout=8, ksize=5) == -2
    assert k(B=1, T=2, H=4, W=4, Cin=32, Cout=8, ksize=3, stride=(3, 1, 1)) == -1
    # the documented routing of the sliding-window predicate: Cout need not be whole pairs of 32-channel blocks
    assert k(B=1, T=2, H=16, W=16, Cin=128, Cout=160, ksize=3) == ("convsw4", False)
    assert k(B=1, T=2, H=16, W=16, Cin=128, Cout=136, ksize=3) == ("convsw4", False)


# ----------------------------------------------------------------------------- GroupNorm kernels
def test_groupnorm_controls_pass_and_a_mutant_fails():
    """the f32 controls of gn_apply (the kernel's expressions from exact sums) and gn_stats (f32 partials per thread) pass on every
    case; the pooled share of apply outputs that differ at all from the f64 statement is what GN_SHARE_CAP is twice of; the scale of
    the neighbouring channel is rejected wherever the variance is not zero"""
    nd = tot = 0
    for C, G, S in VC.GN_CASES:
        c = VC.gn_case(C, G, S)
        VC.check_gn_stats(VC.gn_stats_f32(c), c, "control ")
        for silu in (False, True):
            d, n = VC.check_gn_apply(VC.gn_apply_f32(c, silu), c, silu, "control ")
            nd, tot = nd + d, tot + n
            if S > 1:
                with pytest.raises(AssertionError):
                    VC.check_gn_apply(VC.gn_apply_f32(dict(c, gamma=torch.roll(c["gamma"], 1)), silu), c, silu)
    print(f"gn_apply control: {nd} of {tot} elements differ ({nd / tot:.3e}); cap for the kernel {VC.GN_SHARE_CAP:.3e}")
    assert 2 * nd / tot <= VC.GN_SHARE_CAP * 1.0001


def test_groupnorm_large_mean_control_and_mutant():
    """statistics with |mean| rstd at twice the largest the full-size VAE shows: the rstd from f32-partial sums agrees with the f64
    two-pass rstd to 2^-10; sums whose second moment is one f32 rounding of the whole-tensor total off (no per-thread partials, no
    f64 across blocks) do not"""
    c = VC.gn_case(*VC.GN_BIG_CASE, VC.GN_BIG_RATIO)
    got = float((c["mean"].abs() * c["rstd"]).min())
    assert got >= 0.95 * VC.GN_BIG_RATIO, got
    err = VC.gn_rstd_error(VC.gn_stats_f32(c), c)
    print(f"large-mean control: |mean| rstd {got:.2f}, rstd error {err:.3e} (allowed {VC.GN_RSTD_REL:.3e})")
    assert err <= VC.GN_RSTD_REL
    bad = c["sums"].clone()
    bad[..., 1] *= 1 + 2.0 ** -9            # a second moment kept to bf16 precision
    assert VC.gn_rstd_error(bad, c) > VC.GN_RSTD_REL


# ----------------------------------------------------------------------------- attention_hd512
@pytest.mark.parametrize("name", [c[0] for c in VC.HD_CASES])
def test_hd512_control_passes_and_mutants_fail(name):
    c = VC.hd_case(name)
    rt = VC.hd_reference(c)
    VC.check_hd(VC.hd_control(c), c, rt, "control ")
    with pytest.raises(AssertionError):
        VC.check_hd(VC.hd_control(c, "key_dropped"), c, rt, "mutant key_dropped ")
    if c["masked"]:
        with pytest.raises(AssertionError):
            VC.check_hd(VC.hd_control(c, "mask_shift"), c, rt, "mutant mask_shift ")


def test_guard_bands_catch_a_stray_store():
    """the GPU audit's guard check on host tensors: one element poked into either band fires it"""
    from tests import test_gpu_vae_audit as A
    from tests.test_gpu_row_kernels import _SENTINEL

    n, off = 100, 4
    for pos in (0, A.GUARD + off - 1, A.GUARD + off + n, 2 * A.GUARD + off + n - 1):
        flat = torch.full((2 * A.GUARD + off + n,), _SENTINEL[2], dtype=torch.int16).view(torch.bfloat16)
        A.assert_guards(flat, n, off, "clean")
        flat[pos] = 1.0
        with pytest.raises(AssertionError):
            A.assert_guards(flat, n, off, "poked")
