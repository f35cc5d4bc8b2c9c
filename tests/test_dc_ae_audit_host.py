"""CPU: the launch auditor of the Video DC-AE decoder (tests/dc_ae_audit.py) audited itself.

- clean runs over the CPU emulation of the kernels (tests/cpu_ops_dc_ae.py): every launch passes and the launch census is what
  the architecture implies, at the SMALL widths and at the shipped widths on latent 2 x 4 x 4;
- five deliberately wrong kernel tables, each a patch of ONE entry point made inside this file: the audit must fail, at that
  entry point and at no other.  This is the standing proof that the GPU tests built on the auditor (tests/test_gpu_dc_ae_tile.py)
  fail on a subtly wrong kernel; it needs no mutated GPU build;
- the fallback condition of the auditor (the f32 control itself outside the bound at no more than 10 % of the launches) for
  the weight seed (1) and the reduced latents the GPU tests use.  The emulation table IS the control (f32 formula, one rounding),
  so what these runs measure is the control alone.
"""
import types

import pytest
import torch
import torch.nn.functional as F

from tests import cpu_ops_dc_ae as E
from tests import dc_ae_restatement as R
from tests.dc_ae_audit import BF, FALLBACK_SHARE, Auditor, _judge, expected_census, measure
from tests.test_dc_ae_host import small_model


@pytest.fixture()
def dc_ae(hip_lib):
    from open_sora_amd import dc_ae, mmdit

    yield dc_ae
    mmdit.set_ops_for_testing(hip_lib)


def _audited_decode(dc_ae, model, z, table=E):
    from open_sora_amd import mmdit

    aud = Auditor(table)
    mmdit.set_ops_for_testing(aud)
    with torch.no_grad():
        out = model.decode(z)
    return aud, out


def _latent(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(BF)


def _cases(c):
    return {k: v for k, v in c.items() if v}


# ------------------------------------------------------------------------------------------------------------------ clean runs
@pytest.mark.parametrize("shape", [(1, 32, 3, 4, 5), (1, 32, 1, 3, 4)], ids=["video", "single_frame"])
def test_clean_audit_small_widths(dc_ae, shape):
    aud, out = _audited_decode(dc_ae, small_model(dc_ae, BF), _latent(shape, 11))
    print(aud.report())
    aud.check("emulated SMALL decode")
    assert aud.census() == _cases(expected_census(R.SMALL))
    assert tuple(out.shape) == (1, 3, shape[2] * 4 if shape[2] > 1 else 1, shape[3] * 32, shape[4] * 32)


def test_clean_audit_shipped_widths_reduced_latent(dc_ae):
    """the weights (seed 1) and the latent (seed 5) of tests/test_gpu_dc_ae.py::test_decode_shipped_widths_reduced_latent"""
    with torch.device("cpu"):
        m = dc_ae.DCAE(dc_ae.dc_ae_f32("dc-ae-f32t4c128", None)).to(BF)
    m.load_state_dict(R.make_state_dict(R.param_shapes(R.SHIPPED), seed=1))
    aud, out = _audited_decode(dc_ae, m, _latent((1, 128, 2, 4, 4), 5))
    print(aud.report())
    aud.check("emulated shipped-width decode, latent 2 x 4 x 4")
    want = expected_census(R.SHIPPED)
    assert aud.census() == _cases(want)
    assert want["conv3d_zp/k3"] == 25 and sum(want.values()) == len(aud.records) == 140
    assert aud.fallback_share() <= FALLBACK_SHARE
    assert tuple(out.shape) == (1, 3, 8, 128, 128)


def test_tiled_decode_audits_the_blends(dc_ae):
    m = small_model(dc_ae, BF, use_spatial_tiling=True, use_temporal_tiling=True, spatial_tile_size=128, temporal_tile_size=16)
    aud, out = _audited_decode(dc_ae, m, _latent((1, 32, 5, 5, 6), 12))
    aud.check("emulated SMALL tiled decode")
    c = aud.census()
    tiles = 2 * 2 * 2                                          # steps of 3 latent over 5 / 5 / 6
    one = expected_census(R.SMALL)
    assert c["blend"] == 2 * (2 + 2) + 1                       # per temporal tile: 2 vertical + 2 horizontal; 1 temporal
    assert all(c[k] == tiles * v for k, v in one.items() if v)


# ---------------------------------------------------------------------------------------------------------------------- mutants
def _patched(**fns):
    t = types.SimpleNamespace(**{k: getattr(E, k) for k in dir(E) if not k.startswith("__")})
    for k, f in fns.items():
        setattr(t, k, f)
    return t


def _conv_variant(pad_mode="constant", silu_before_bias=False):
    def conv3d_zp(x, w, bias, out, ksize, up_t=False, up_hw=False, silu=False, res=None):
        B, T, H, W, Cin = x.shape
        Cout = w.shape[0]
        wk = w[:, : ksize ** 3 * Cin].float().reshape(Cout, ksize, ksize, ksize, Cin).permute(0, 4, 1, 2, 3)
        xs = x.float().permute(0, 4, 1, 2, 3)
        if up_t:
            xs = xs.repeat_interleave(2, 2)
        if up_hw:
            xs = xs.repeat_interleave(2, 3).repeat_interleave(2, 4)
        p = ksize // 2
        if p:
            xs = F.pad(xs, (p,) * 6, mode=pad_mode)
        y = F.conv3d(xs, wk)
        b = 0.0 if bias is None else bias.float().view(1, -1, 1, 1, 1)
        if silu_before_bias:
            y = (F.silu(y) if silu else y) + b
        else:
            y = y + b
            y = F.silu(y) if silu else y
        y = y.permute(0, 2, 3, 4, 1)
        if res is not None:
            y = y + res.float()
        out.copy_(y.to(out.dtype))
        return out

    return conv3d_zp


def _dup_hw_swapped(x, out, ft, fhw):
    B, T, H, W, Cin = x.shape
    Cout = out.shape[-1]
    rep = Cout * ft * fhw * fhw // Cin
    t = torch.arange(T * ft).view(-1, 1, 1, 1)
    h = torch.arange(H * fhw).view(1, -1, 1, 1)
    w = torch.arange(W * fhw).view(1, 1, -1, 1)
    co = torch.arange(Cout).view(1, 1, 1, -1)
    ci = (((co * ft + t % ft) * fhw + w % fhw) * fhw + h % fhw) // rep        # h and w sub-indices swapped
    out.copy_(x[:, t // ft, h // fhw, w // fhw, ci])
    return out


def _rms_res_before_relu(x, weight, bias, out, eps=1e-5, res=None, relu=False):
    xs = x.float()
    y = xs * torch.rsqrt(xs.square().mean(-1, keepdim=True) + eps) * weight + bias
    if res is not None:
        y = y + res.float()
    if relu:
        y = torch.relu(y)
    out.copy_(y.to(out.dtype))
    return out


def _attn_last_run_dropped(qkv, out, eps=1e-15, workspace=None):
    """the K^T V sum stops one 64-token run short of N"""
    B, N, C3 = qkv.shape
    g = qkv.float().reshape(B, N, C3 // 96, 96).permute(0, 2, 1, 3)
    q, k, v = torch.relu(g[..., :32]), torch.relu(g[..., 32:64]), g[..., 64:]
    keep = (N - 1) // 64 * 64 if N > 64 else N
    v1 = torch.cat([v, torch.ones_like(v[..., :1])], -1)[:, :, :keep]
    kv = v1.transpose(-1, -2) @ k[:, :, :keep]
    o = q @ kv.transpose(-1, -2)
    o = o[..., :32] / (o[..., 32:] + eps)
    out[:, :, : C3 // 3].copy_(o.permute(0, 2, 1, 3).reshape(B, N, C3 // 3).to(out.dtype))
    return out


def test_the_unmutated_variants_are_clean(dc_ae):
    """the mutants' scaffolding itself (a conv through F.conv3d with the CORRECT padding and order) passes the audit, so a
    mutant's failure is the mutation's"""
    aud, _ = _audited_decode(dc_ae, small_model(dc_ae, BF), _latent((1, 32, 3, 4, 5), 11), _patched(conv3d_zp=_conv_variant()))
    aud.check("scaffolding")


MUTANTS = [
    ("silu_before_bias", "conv3d_zp", dict(conv3d_zp=_conv_variant(silu_before_bias=True))),
    ("replicate_padding", "conv3d_zp", dict(conv3d_zp=_conv_variant(pad_mode="replicate"))),
    ("dup_shuffle_hw_swapped", "dup_shuffle", dict(dup_shuffle=_dup_hw_swapped)),
    ("attn_last_run_dropped", "relu_linear_attn", dict(relu_linear_attn=_attn_last_run_dropped)),
]


@pytest.mark.parametrize("name,entry,patch", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant_is_caught_at_its_entry_point(dc_ae, name, entry, patch):
    aud, _ = _audited_decode(dc_ae, small_model(dc_ae, BF), _latent((1, 32, 3, 4, 5), 11), _patched(**patch))
    bad = aud.failures()
    assert bad, f"{name}: the audit passed a wrong kernel table"
    assert {r["entry"] for r in bad} == {entry}, [(r["n"], r["entry"]) for r in bad]
    with pytest.raises(AssertionError, match=rf"first: launch {bad[0]['n']} \({entry}\)") as ei:
        aud.check(name)
    text = str(ei.value)
    assert text.count("FAIL:") == len(bad)                    # every failure of the decode, not the first alone
    if entry == "conv3d_zp":
        assert "worst element (b=0, t=" in text and ("on a border" in text or "in the interior" in text)
    if name == "replicate_padding":                          # only padded faces can differ
        assert "in the interior" not in text and all("border" in r["why"] for r in bad)


def test_mutant_residual_before_relu_is_caught(dc_ae):
    """the decoder never asks rmsnorm_affine for ReLU and a residual together (project_out has no shortcut), so a decode cannot
    see this mutant; the ABI allows the pair, and the auditor is driven with it directly"""
    aud = Auditor(_patched(rmsnorm_affine=_rms_res_before_relu))
    g = torch.Generator().manual_seed(3)
    x, r = (3 * torch.randn(2, 3, 4, 5, 64, generator=g)).to(BF), torch.randn(2, 3, 4, 5, 64, generator=g).to(BF)
    w, b = 1 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g)
    aud.rmsnorm_affine(x, w, b, torch.empty_like(x), 1e-5, None, True)      # either flag alone: the mutant is right
    aud.rmsnorm_affine(x, w, b, torch.empty_like(x), 1e-5, r, False)
    assert not aud.failures()
    aud.rmsnorm_affine(x, w, b, torch.empty_like(x), 1e-5, r, True)
    bad = aud.failures()
    assert [(f["n"], f["entry"]) for f in bad] == [(2, "rmsnorm_affine")]
    with pytest.raises(AssertionError, match=r"first: launch 2 \(rmsnorm_affine\)"):
        aud.check()


# ------------------------------------------------------------------------------------------------------------- the auditor's parts
def test_unaudited_entry_points_are_refused():
    aud = Auditor(E)
    with pytest.raises(AttributeError, match="not audited"):
        aud.gemm_pair
    assert aud.BF is E.BF                                      # constants pass through


def test_fallback_route_and_its_cap():
    """a launch whose f32 control misses the bound is judged by 2 x control, named, and counted; more than 10 % of them fail
    check().  Crafted tensors: the control is off by 1e-2 max|y| everywhere."""
    y = torch.randn(64, 64, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    d = 1e-2 * float(y.abs().max())
    aud = Auditor(E)
    aud._record("gemm", "gemm", "crafted: kernel 1.5 x control", y + 1.5 * d, y, y + d)
    assert aud.records[0]["ok"] and aud.records[0]["route"] == "fallback"
    aud._record("gemm", "gemm", "crafted: kernel 3 x control", y + 3 * d, y, y + d)
    assert not aud.records[1]["ok"] and "2 x control" in aud.records[1]["why"]
    aud._record("gemm", "gemm", "crafted: control inside, kernel outside", y + d, y, y)
    assert not aud.records[2]["ok"] and aud.records[2]["route"] == "control" and "bound rule" in aud.records[2]["why"]
    aud = Auditor(E)
    aud._record("gemm", "gemm", "crafted", y + 1.5 * d, y, y + d)
    for _ in range(8):
        aud._record("gemm", "gemm", "exact", y, y, y)
    with pytest.raises(AssertionError, match="control itself misses the bound"):
        aud.check()                                            # 1 of 9 launches > 10 %
    aud._record("gemm", "gemm", "exact", y, y, y)
    aud.check()                                                # 1 of 10
    assert "1 judged by the 2 x control fallback (10.0 %" in aud.report()


def test_judge_is_the_bound():
    y = torch.linspace(-4, 4, 4096, dtype=torch.float64).reshape(64, 64)
    _judge("rounded once", y.to(BF), y)
    with pytest.raises(AssertionError, match="off by"):
        _judge("2^-7 relative", (y * (1 + 2.0 ** -7)).float(), y)
    bad = y.clone()
    bad[0, 5] += 1.0
    border = torch.zeros(64, 64, dtype=torch.bool)
    border[0] = True
    with pytest.raises(AssertionError, match="border voxels"):
        _judge("one border element", bad.float(), y, border)
    m = measure(bad.float(), y, border)
    assert m["worst"] == ((0, 5), True) and m["regions"]["interior"][1]
