"""GPU: the CLIP text encoder (open_sora_amd.clip; csrc/layernorm.hip, the CAUSAL instantiation of csrc/attention_relbias.hip, the
quick-GELU instantiation of csrc/gemm_bf16.hip) on the MI355X.

Every kernel is judged by tests.util.assert_parity: the truth is an fp64 (models: fp32) evaluation on the CPU of the formula of
include/osk.h from bf16-representable inputs, the comparator torch's own bf16 evaluation of the same formula.  Outputs lie inside
larger sentinel-filled buffers: nothing outside the view may change.
- causal attention: one tile, the diagonal tile with a tail, a skipped tile, a fused q|k|v buffer; causality as a property (keys
  and values behind position p do not reach rows <= p, bit for bit); an unsupported head dim;
- LayerNorm: the two widths of the models, padded row strides, a constant row (bf16(bias) exactly), rows of nearly equal values;
- quick-GELU GEMM: the model's shapes and a scalar column tail, with proof that the check tells quick-GELU from tanh-GELU, and the
  plain GEMM's tanh-GELU unchanged behind it;
- the small-geometry encoder against the fp32 restatement (tests/clip_restatement.py) and against the output transformers recorded
  (tests/golden/clip_small.npz); one layer at the width of CLIP-L at 231 and at 385 rows."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import clip_restatement as R
from tests import cpu_ops_clip as E
from tests.util import assert_parity, finite_retry
from tools.make_golden_clip import small_state_dict

BF = torch.bfloat16
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_small.npz")
SENTINEL = 7.0


@pytest.fixture()
def clip(hip_lib):
    from open_sora_amd import clip, mmdit

    mmdit.set_ops_for_testing(hip_lib)
    torch.cuda.set_device(0)
    return clip


# ------------------------------------------------------------------------------------------------------- causal attention
def _operands(B, L, H, layout, seed):
    """q, k, v (bf16 views on the device), seeded on the CPU; scores of a few units, so that the softmax is far from uniform"""
    g = torch.Generator().manual_seed(seed)
    C = H * 64
    if layout == "fused":                      # one [B, L, 3 C] projection output, q | k | v read in place
        qkv = torch.randn(B, L, 3 * C, generator=g)
        qkv[:, :, : 2 * C] *= 2.0
        qkv = qkv.to(BF).to(DEV)
        return qkv[:, :, :C], qkv[:, :, C: 2 * C], qkv[:, :, 2 * C:]
    q, k = ((2.0 * torch.randn(B, L, C, generator=g)).to(BF).to(DEV) for _ in range(2))
    return q, k, torch.randn(B, L, C, generator=g).to(BF).to(DEV)


def _guarded(shape, pad_rows=3, pad_cols=24, left=8):
    """a bf16 view of `shape` inside a larger sentinel-filled buffer, and a mask of the elements outside it"""
    *lead, rows, cols = shape
    big = torch.full((*lead, rows + pad_rows, cols + pad_cols), SENTINEL, dtype=BF, device=DEV)
    outside = torch.ones_like(big, dtype=torch.bool)
    outside[..., 1: 1 + rows, left: left + cols] = False
    return big, big[..., 1: 1 + rows, left: left + cols], outside


def _untouched(big, outside):
    return bool((big[outside] == SENTINEL).all())


def _check_attention(hip_lib, name, B, L, H, layout, scale=0.125):
    q, k, v = _operands(B, L, H, layout, seed=2000 + L + 7 * H)
    big, out, outside = _guarded((B, L, H * 64))
    hip_lib.attention_causal(q, k, v, out, H, 64, scale)
    torch.cuda.synchronize()
    assert _untouched(big, outside), f"{name}: wrote outside the [B, L, H * 64] view of out"
    truth = E.attention_causal_ref(q.cpu(), k.cpu(), v.cpu(), H, 64, scale, dtype=torch.float64)
    ref_bf16 = E.attention_causal_ref(q, k, v, H, 64, scale, dtype=BF)                 # torch's own bf16 arithmetic, on the device
    assert_parity(out, truth, ref_bf16, name)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 63, 64, 65, 77, 130])
def test_causal_attention_tiles(hip_lib, L):
    """one tile (1, 63, 64), the diagonal tile with a tail (65, 77), a tile above the diagonal that query block 0 skips (130)"""
    _check_attention(hip_lib, f"causal L={L}", 1, L, 1, "contiguous")


@pytest.mark.gpu
def test_causal_attention_fused_qkv(hip_lib):
    _check_attention(hip_lib, "causal L=200 fused qkv", 3, 200, 3, "fused")


@pytest.mark.gpu
def test_causal_attention_never_reads_behind_the_query(hip_lib):
    """keys and values at positions > p, overwritten with large finite numbers (a NaN would survive a zero probability in the
    MFMA), leave the rows <= p bit-identical"""
    B, L, H = 2, 130, 2
    q, k, v = _operands(B, L, H, "contiguous", seed=77)
    first = hip_lib.attention_causal(q, k, v, torch.empty_like(q), H, 64, 0.125).clone()
    for p in (0, 63, 64, 76):
        k2, v2 = k.clone(), v.clone()
        k2[:, p + 1:] = 3.0e4
        v2[:, p + 1:] = -3.0e4
        out = hip_lib.attention_causal(q, k2, v2, torch.empty_like(q), H, 64, 0.125)
        torch.cuda.synchronize()
        assert torch.equal(out[:, : p + 1], first[:, : p + 1]), f"p = {p}: a row <= p changed"
        assert bool(torch.isfinite(out.float()).all()) and not torch.equal(out[:, p + 1:], first[:, p + 1:])


@pytest.mark.gpu
def test_causal_attention_unsupported_head_dim_writes_nothing(hip_lib):
    B, L, H, hd = 1, 64, 2, 72
    q, k, v = (torch.randn(B, L, H * hd, device=DEV).to(BF) for _ in range(3))
    out = torch.full((B, L, H * hd), SENTINEL, dtype=BF, device=DEV)
    rc = hip_lib.lib.osk_attention_causal_bf16(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1),
                                               v.data_ptr(), v.stride(0), v.stride(1), out.data_ptr(), out.stride(0), out.stride(1),
                                               B, H, L, hd, 1.0, None)
    torch.cuda.synchronize()
    assert rc == hip_lib.OSK_EUNSUPPORTED == -2
    assert bool((out == SENTINEL).all())
    with pytest.raises(RuntimeError, match="osk_attention_causal_bf16 failed: status -2"):
        hip_lib.attention_causal(q, k, v, out, H, hd, 1.0)
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------- LayerNorm
def _ln_case(hip_lib, name, x, w, b, eps=1e-5):
    """x bf16 [M, C] view on the device; w, b f32 with bf16-representable values.  Returns the kernel's output."""
    M, C = x.shape
    big, out, outside = _guarded((M, C), pad_rows=2, pad_cols=16)
    hip_lib.layernorm_affine(x, w, b, out, eps)
    torch.cuda.synchronize()
    assert _untouched(big, outside), f"{name}: wrote outside the [M, C] view of out"
    truth = E.layernorm_affine_ref(x.cpu(), w.cpu(), b.cpu(), eps, dtype=torch.float64)
    ref_bf16 = F.layer_norm(x, (C,), w.to(BF), b.to(BF), eps)                          # torch's own bf16 LayerNorm, on the device
    assert_parity(out, truth, ref_bf16, name)
    return out


def _ln_params(C, g):
    return (1.0 + 0.25 * torch.randn(C, generator=g)).to(BF).float().to(DEV), (0.5 * torch.randn(C, generator=g)).to(BF).float().to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("M,C,row_stride", [(1, 128, 128), (231, 768, 768), (5, 768, 808)])
def test_layernorm_against_f64(hip_lib, M, C, row_stride):
    g = torch.Generator().manual_seed(M + C)
    x = (1.5 * torch.randn(M, row_stride, generator=g) + 0.75).to(BF).to(DEV)[:, :C]
    assert x.stride(0) == row_stride
    _ln_case(hip_lib, f"layernorm {M}x{C} (row stride {row_stride})", x, *_ln_params(C, g))


@pytest.mark.gpu
def test_layernorm_constant_row_is_the_bias(hip_lib):
    """a constant row of 300: the variance of the centred values is exactly 0 (E[x^2] - mean^2 would not be: 90000 - 90000 in f32
    may come out negative, and rsqrt of it NaN), so the row comes out as bf16(bias), finite"""
    g = torch.Generator().manual_seed(3)
    for C in (128, 768):
        w, b = _ln_params(C, g)
        x = torch.randn(6, C, generator=g).to(BF).to(DEV)
        x[1] = 300.0
        x[4] = -300.0
        out = _ln_case(hip_lib, f"layernorm constant rows, C = {C}", x, w, b)
        assert bool(torch.isfinite(out.float()).all())
        assert torch.equal(out[1], b.to(BF)) and torch.equal(out[4], b.to(BF))


@pytest.mark.gpu
def test_layernorm_nearly_constant_rows(hip_lib):
    """rows drawn from {254, 256, 258}: a mean of 256 under deviations of 2 -- the one-pass variance loses all of its digits here"""
    g = torch.Generator().manual_seed(4)
    x = (254.0 + 2.0 * torch.randint(0, 3, (9, 768), generator=g)).to(BF).to(DEV)
    _ln_case(hip_lib, "layernorm rows of {254, 256, 258}", x, *_ln_params(768, g))


@pytest.mark.gpu
def test_layernorm_unsupported_width_writes_nothing(hip_lib):
    x = torch.randn(4, 132, device=DEV).to(BF)
    out = torch.full((4, 132), SENTINEL, dtype=BF, device=DEV)
    w = torch.ones(132, device=DEV)
    with pytest.raises(RuntimeError, match="osk_layernorm_affine_bf16 failed: status -"):
        hip_lib.layernorm_affine(x, w, w, out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------- quick-GELU GEMM
def _gelu_tanh64(v):
    return F.gelu(v, approximate="tanh")


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(77, 512, 128), (231, 3072, 768), (385, 3072, 768), (50, 258, 64)])
def test_gemm_quickgelu_against_f64(hip_lib, M, N, K):
    """pre-activations of standard deviation about 2: both tails and the dip of the activation are populated.  N = 258 takes the
    scalar column tail of the epilogue (its row stride, 260, keeps the 8-byte alignment the entry asks for)."""
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(1, M, K, generator=g).to(BF).to(DEV)
    w = (2.0 * K ** -0.5 * torch.randn(N, K, generator=g)).to(BF).to(DEV)
    bias = (0.5 * torch.randn(N, generator=g)).to(BF).float().to(DEV)
    Np = (N + 3) // 4 * 4
    big = torch.full((1, M + 2, Np + 8), SENTINEL, dtype=BF, device=DEV)
    out = big[:, 1: 1 + M, 4: 4 + N]
    outside = torch.ones_like(big, dtype=torch.bool)
    outside[:, 1: 1 + M, 4: 4 + N] = False
    name = f"gemm_quickgelu {M}x{N}x{K}"
    hip_lib.gemm_quickgelu(a, w, bias, out)
    torch.cuda.synchronize()
    assert _untouched(big, outside), f"{name}: wrote outside the [M, N] view of out"
    pre = a.cpu().double() @ w.cpu().double().T + bias.cpu().double()
    assert 1.5 < float(pre.std()) < 2.6
    truth = E.quick_gelu_ref(pre)
    ref_bf16 = E.quick_gelu_ref(F.linear(a, w, bias.to(BF)))                           # torch's own bf16 arithmetic, on the device
    assert_parity(out, truth, ref_bf16, name)
    # the check can tell the two activations apart: the EXACT tanh-GELU of the same pre-activations does not pass it
    with pytest.raises(AssertionError, match="relL2 ours"):
        assert_parity(_gelu_tanh64(pre), truth, ref_bf16, name + " (tanh-GELU in place of quick-GELU)")
    # and the plain entry's tanh-GELU is what it was
    out2 = torch.empty(1, M, Np, dtype=BF, device=DEV)[:, :, :N]
    hip_lib.gemm(a, w, bias, out2, gelu_from=0)
    torch.cuda.synchronize()
    assert_parity(out2, _gelu_tanh64(pre), _gelu_tanh64(F.linear(a, w, bias.to(BF))), f"gemm gelu_from=0 {M}x{N}x{K}")
    with pytest.raises(AssertionError, match="relL2 ours"):
        assert_parity(out2, truth, ref_bf16, name + " (the plain entry is not quick-GELU)")


# ------------------------------------------------------------------------------------------------------------------- model
def _restated(cfg, sd, ids, dtype, device="cpu"):
    sd = {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}
    with torch.no_grad():
        return R.encode(sd, cfg, ids.to(device))


@pytest.mark.gpu
def test_small_encoder_against_restatement_and_golden(clip):
    golden = np.load(GOLDEN)
    ids = torch.from_numpy(golden["input_ids"])
    sd = small_state_dict()
    m = clip.ClipTextModel(clip.ClipTextConfig(**R.SMALL)).to(BF).to(DEV)
    m.load_state_dict({k: v.to(BF) for k, v in sd.items()})
    out = m(input_ids=ids.to(DEV), attention_mask=None, output_hidden_states=False)
    y, pooled = out["last_hidden_state"], out["pooler_output"]
    torch.cuda.synchronize()
    assert y.dtype == pooled.dtype == BF and tuple(y.shape) == (3, 77, 128) and tuple(pooled.shape) == (3, 128) and y.device.type == "cuda"
    y32, p32 = _restated(R.SMALL, sd, ids, torch.float32)
    y16, p16 = _restated(R.SMALL, sd, ids, BF)
    if not bool(torch.isfinite(y16.float()).all()):
        y16 = finite_retry(lambda: _restated(R.SMALL, sd, ids, BF)[0])
    assert_parity(y, y32, y16, "clip small encoder vs restatement")
    assert_parity(pooled, p32, p16, "clip small pooler_output vs restatement")
    assert_parity(y, torch.from_numpy(golden["last_hidden_state"]), torch.from_numpy(golden["last_hidden_state_bf16_bits"]).view(BF),
                  "clip small encoder vs transformers' recorded output")
    assert_parity(pooled, torch.from_numpy(golden["pooler_output"]), torch.from_numpy(golden["pooler_output_bf16_bits"]).view(BF),
                  "clip small pooler_output vs transformers' recorded output")
    again = m(ids.to(DEV))                                          # the cached plan and workspace: bit-identical
    assert torch.equal(again.last_hidden_state, y) and torch.equal(again.pooler_output, pooled)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 5])
def test_one_full_width_layer(clip, hip_lib, B):
    """hidden 768, 12 heads, intermediate 3072 at L = 77: the GEMM shapes of CLIP-L; B = 5 is 385 rows, where the plain GEMMs may
    take the 256-row tiles (the quick-GELU entry never does)"""
    cfg = R.L_LAYER
    sd = R.make_state_dict(cfg, seed=1)
    top = cfg["vocab_size"] - 1
    ids = torch.randint(0, top, (B, 77), generator=torch.Generator().manual_seed(4 + B))
    ids[torch.arange(B), torch.arange(B) * 15 + 9] = top
    with torch.device(DEV):
        m = clip.ClipTextModel(clip.ClipTextConfig(**cfg)).to(BF)
    m.load_state_dict({k: v.to(BF) for k, v in sd.items()})
    out = m(ids.to(DEV))
    torch.cuda.synchronize()
    print(f"{B * 77} rows; gemm tile kinds at >= 256 rows (1 = 256 x 128; fewer rows always take 128 x 128):",
          {n: hip_lib.lib.osk_gemm_tile_choice(B * 77, *nk) for n, nk in dict(qkv=(2304, 768), o=(768, 768), fc2=(768, 3072)).items()})
    y32, p32 = _restated(cfg, sd, ids, torch.float32)               # fp32 on the CPU
    y16, p16 = _restated(cfg, sd, ids, BF, device=DEV)              # torch's own bf16 arithmetic, on the device
    assert_parity(out.last_hidden_state, y32, y16, f"clip one L-width layer, B = {B}")
    assert_parity(out.pooler_output, p32, p16, f"clip one L-width layer pooler_output, B = {B}")
    assert all(torch.equal(out.pooler_output[b], out.last_hidden_state[b, 15 * b + 9]) for b in range(B))
