"""GPU: the T5 text encoder (open_sora_amd.t5, csrc/attention_relbias.hip) on the MI355X.

- osk_attention_relbias_bf16 against an fp64 evaluation of the formula of include/osk.h on the CPU (bf16-representable inputs, a
  bias of N(0, 5^2) so that it decides the ranking of the keys); tolerance: tests.util.assert_parity with a bf16 torch evaluation
  of the same formula as the comparator.  `out` lies inside a larger buffer filled with a sentinel: nothing outside the
  [B, L, H * 64] view may change;
- the small-geometry encoder against the fp32 restatement (tests/t5_restatement.py) and against the output transformers recorded
  (tests/golden/t5_small.npz);
- one layer at the width of T5-v1.1-XXL (the 256-row GEMM tiles and the fused GEGLU epilogue) against the restatement in fp32 on
  the CPU, its bf16 run as the comparator."""
import os

import numpy as np
import pytest
import torch

from tests import cpu_ops_t5 as E
from tests import t5_restatement as R
from tests.util import assert_parity, finite_retry
from tools.make_golden_t5 import small_state_dict

BF = torch.bfloat16
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t5_small.npz")
SENTINEL = 7.0


@pytest.fixture()
def t5(hip_lib):
    from open_sora_amd import mmdit, t5

    mmdit.set_ops_for_testing(hip_lib)
    torch.cuda.set_device(0)
    return t5


def _operands(B, L, H, layout, seed, bias_stride=None, with_bias=True):
    """q, k, v (bf16 views on the device), bias (f32 view | None), all seeded on the CPU"""
    g = torch.Generator().manual_seed(seed)
    C = H * 64
    if layout == "fused":                      # one [B, L, 3 C] projection output, q | k | v read in place
        qkv = torch.randn(B, L, 3 * C, generator=g)
        qkv[:, :, : 2 * C] *= 0.5
        qkv = qkv.to(BF).to(DEV)
        q, k, v = qkv[:, :, :C], qkv[:, :, C: 2 * C], qkv[:, :, 2 * C:]
    else:
        q, k = ((0.5 * torch.randn(B, L, C, generator=g)).to(BF).to(DEV) for _ in range(2))
        v = torch.randn(B, L, C, generator=g).to(BF).to(DEV)
    bias = None
    if with_bias:
        stride = bias_stride or 2 * L - 1
        bias = (5.0 * torch.randn(H, stride, generator=g)).to(DEV)[:, : 2 * L - 1]
    return q, k, v, bias


def _guarded_out(B, L, C):
    """out as an interior view of a larger sentinel-filled buffer, and a mask of the elements outside it"""
    big = torch.full((B, L + 3, C + 24), SENTINEL, dtype=BF, device=DEV)
    outside = torch.ones_like(big, dtype=torch.bool)
    outside[:, 1: 1 + L, 8: 8 + C] = False
    return big, big[:, 1: 1 + L, 8: 8 + C], outside


def _check_kernel(hip_lib, name, B, L, H, layout, scale=1.0, bias_stride=None, with_bias=True):
    q, k, v, bias = _operands(B, L, H, layout, seed=1000 + L + 7 * H, bias_stride=bias_stride, with_bias=with_bias)
    if bias_stride:
        assert bias.stride(0) == bias_stride != 2 * L - 1
    big, out, outside = _guarded_out(B, L, H * 64)
    hip_lib.attention_relbias(q, k, v, out, H, 64, scale, bias)
    torch.cuda.synchronize()
    assert bool((big[outside] == SENTINEL).all()), f"{name}: wrote outside the [B, L, H * 64] view of out"
    cpu = [t.cpu() for t in (q, k, v)] + [None if bias is None else bias.cpu()]
    truth = E.attention_relbias_ref(cpu[0], cpu[1], cpu[2], H, 64, scale, cpu[3], dtype=torch.float64)
    ref_bf16 = E.attention_relbias_ref(q, k, v, H, 64, scale, bias, dtype=BF)          # torch's own bf16 arithmetic, on the device
    assert_parity(out, truth, ref_bf16, name)
    return out, truth, (q, k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 63, 64, 65])
def test_relbias_single_and_short_rows(hip_lib, L):
    _check_kernel(hip_lib, f"relbias L={L}", 1, L, 1, "contiguous")


@pytest.mark.gpu
def test_relbias_partial_last_tile_fused_qkv(hip_lib):
    _check_kernel(hip_lib, "relbias L=200 fused qkv", 3, 200, 3, "fused")


@pytest.mark.gpu
def test_relbias_full_tiles_t5_xxl_shape(hip_lib):
    _check_kernel(hip_lib, "relbias L=512 B=2 H=64", 2, 512, 64, "contiguous", bias_stride=2 * 512 + 5)


@pytest.mark.gpu
def test_relbias_tail_on_both_axes(hip_lib):
    _check_kernel(hip_lib, "relbias L=520", 1, 520, 2, "contiguous")


@pytest.mark.gpu
def test_relbias_null_bias_scaled(hip_lib):
    """bias = NULL, scale = 1/8: plain softmax attention against torch fp64 (none of the large attention kernels involved)"""
    _, truth, (q, k, v) = _check_kernel(hip_lib, "relbias L=200 no bias, scale 1/8", 3, 200, 3, "fused", scale=0.125, with_bias=False)
    qh, kh, vh = (t.cpu().double().reshape(3, 200, 3, 64).transpose(1, 2) for t in (q, k, v))
    plain = (torch.softmax(qh @ kh.transpose(2, 3) * 0.125, -1) @ vh).transpose(1, 2).reshape(3, 200, 192)
    assert float((plain - truth).abs().max()) <= 1e-12


@pytest.mark.gpu
def test_relbias_unsupported_head_dim_writes_nothing(hip_lib):
    B, L, H, hd = 1, 64, 2, 72
    q, k, v = (torch.randn(B, L, H * hd, device=DEV).to(BF) for _ in range(3))
    out = torch.full((B, L, H * hd), SENTINEL, dtype=BF, device=DEV)
    bias = torch.zeros(H, 2 * L - 1, device=DEV)
    rc = hip_lib.lib.osk_attention_relbias_bf16(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1),
                                                v.data_ptr(), v.stride(0), v.stride(1), out.data_ptr(), out.stride(0), out.stride(1),
                                                bias.data_ptr(), bias.stride(0), B, H, L, hd, 1.0, None)
    torch.cuda.synchronize()
    assert rc == hip_lib.OSK_EUNSUPPORTED == -2
    assert bool((out == SENTINEL).all())
    with pytest.raises(RuntimeError, match="osk_attention_relbias_bf16 failed: status -2"):
        hip_lib.attention_relbias(q, k, v, out, H, hd, 1.0, bias)
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------- model
def _restated(cfg, sd, ids, dtype, device="cpu"):
    sd = {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}
    with torch.no_grad():
        return R.encode(sd, cfg, ids.to(device))


@pytest.mark.gpu
def test_small_encoder_against_restatement_and_golden(t5):
    golden = np.load(GOLDEN)
    ids = torch.from_numpy(golden["input_ids"])
    sd = small_state_dict()
    m = t5.T5Encoder(t5.T5EncoderConfig(**R.SMALL)).to(BF).to(DEV)
    m.load_state_dict({k: v.to(BF) for k, v in sd.items()})
    out = m(input_ids=ids.to(DEV), attention_mask=None, output_hidden_states=False)["last_hidden_state"]
    torch.cuda.synchronize()
    assert out.dtype == BF and tuple(out.shape) == (2, 192, 256) and out.device.type == "cuda"
    assert_parity(out, _restated(R.SMALL, sd, ids, torch.float32), finite_retry(lambda: _restated(R.SMALL, sd, ids, BF)),
                  "t5 small encoder vs restatement")
    assert_parity(out, torch.from_numpy(golden["last_hidden_state"]), torch.from_numpy(golden["last_hidden_state_bf16_bits"]).view(BF),
                  "t5 small encoder vs transformers' recorded output")
    again = m(ids.to(DEV)).last_hidden_state                        # the cached plan and workspace: bit-identical
    assert torch.equal(again, out)


@pytest.mark.gpu
def test_one_full_width_layer(t5, hip_lib):
    """d_model 4096, 64 heads, d_ff 10240 at B = 2, L = 512: the GEMM shapes of T5-v1.1-XXL"""
    cfg = R.XXL_LAYER
    sd = R.make_state_dict(cfg, seed=1, device=DEV)                 # generated on the device (0.2 G parameters)
    ids = torch.randint(0, cfg["vocab_size"], (2, 512), generator=torch.Generator().manual_seed(4))
    with torch.device(DEV):
        m = t5.T5Encoder(t5.T5EncoderConfig(**cfg)).to(BF)
    m.load_state_dict({k: v.to(BF) for k, v in sd.items()})
    out = m(ids.to(DEV)).last_hidden_state
    torch.cuda.synchronize()
    kinds = {n: hip_lib.lib.osk_gemm_tile_choice(1024, *nk) for n, nk in
             dict(qkv=(12288, 4096), o=(4096, 4096), wi=(20480, 4096), wo=(4096, 10240)).items()}
    print("gemm tile kinds (2 = 256 x 256):", kinds)
    assert kinds["qkv"] == 2 and kinds["wi"] == 2, kinds            # the 256 x 256 tile and the fused GEGLU epilogue ran above
    truth = _restated(cfg, sd, ids, torch.float32)                  # fp32 on the CPU
    ref_bf16 = _restated(cfg, sd, ids, BF, device=DEV)              # torch's own bf16 arithmetic, on the device
    assert_parity(out, truth, ref_bf16, "t5 one XXL-width layer")
