"""GPU tests of the head_dim-128 attention with QK^T AND P.V on the fp8 MFMA (osk_k_pack_fp8, osk_attention_fwd_qk8_bf16,
MMDiTModel.enable_fp8(qk8=True)).

Three results per kernel case:
  ref    exact f64 attention on the bf16 operands;
  ref_q  f64 attention on the KERNEL'S OWN operands -- K dequantised from the rule of include/osk.h (one scale per (key batch, head)),
         Q dequantised from the per-(row, head) rule, V as the kernel's e4m3 V, P exact.  This is the yardstick that isolates the
         kernel: what remains between it and the kernel is P's e4m3 rounding, the noise the project bounds at 4e-2 for pv8;
  out    the kernel.
rel(out, ref) and rel(ref_q, ref) are printed for every case (profiles/attn_qk8.md records them); the fp8 QK^T error itself is a
property of the format and the inputs, so only the triangle bound rel(out, ref) <= rel(ref_q, ref) + 4e-2 (+ 1e-3 for the ratio of
the two norms) is asserted on it.
"""
import pytest
import torch

from tests.test_gpu_kernels import BF, DEV, rnd

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
HD = 128
LOG2E = 1.4426950408889634


def _fix0(t):
    """-0 and +0 are the same e4m3 value"""
    return torch.where(t == 0x80, torch.zeros_like(t), t)


def _k_scales(k, H):
    """k [n_seg, B, seg, D] -> f32 [B, H]: absmax over all segments / 448 (1.0 for an all-zero head)"""
    n_seg, B, seg, _ = k.shape
    amax = k.float().abs().view(n_seg, B, seg, H, HD).amax(dim=(0, 2, 4)).cpu()   # the division on the CPU: IEEE, like the kernel's
    return torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)).contiguous().to(k.device)


def _pack_ref(k, s, H):
    """torch restatement of osk_k_pack_fp8 on the CPU: k bf16 [B, L, H*128], s f32 [B, H] -> uint8 [B, H, Lp, 128]"""
    B, L, _ = k.shape
    Lp = (L + 63) // 64 * 64
    kf = k.float().cpu().view(B, L, H, HD).permute(0, 2, 1, 3)
    q8 = (kf / s.cpu()[:, :, None, None]).clamp(-448.0, 448.0).to(F8).view(torch.uint8)
    return torch.cat([q8, q8[:, :, L - 1:L].expand(B, H, Lp - L, HD)], 2).contiguous()


@pytest.mark.parametrize("B,H,L", [(2, 2, 65), (1, 24, 333), (2, 3, 704)])
def test_k_pack_fp8_bit_exact(hip_lib, B, H, L):
    D = H * HD
    y = rnd("y", (B, L + 3, 3 * D), std=1.3, seed=171)
    k = y[:, 3:, D: 2 * D]                           # strided view inside a fused projection buffer
    k[0, :, :HD] = 0                                 # an all-zero head: scale 1, bytes 0
    k[B - 1, L // 2, D - 5] = 200.0                  # an outlier that owns its head's scale
    s = hip_lib.v_scale_fp8(k, H, HD)
    k8 = torch.full(hip_lib.k8_shape(B, H, L), 0xAA, dtype=torch.uint8, device=DEV)
    hip_lib.k_pack_fp8(k, s, k8, H, HD)
    assert torch.equal(s.cpu(), _k_scales(k[None], H).cpu())
    ref = _pack_ref(k, s, H)
    assert torch.equal(_fix0(k8.cpu()), _fix0(ref))
    assert torch.equal(k8[:, :, L:], k8[:, :, L - 1:L].expand(B, H, k8.shape[2] - L, HD))   # the tail repeats the last key


def _operands(hip_lib, B, H, Lq, Lk, n_seg, Bkv, spike, seed, const_v=None):
    D = H * HD
    seg = Lk // n_seg
    q = rnd("q", (B, Lq, D), seed=seed)
    k = rnd("k", (n_seg, Bkv, seg, D), seed=seed + 1)
    v = rnd("v", (n_seg, Bkv, seg, D), seed=seed + 2) if const_v is None else const_v[None, None, None].expand(n_seg, Bkv, seg, D).contiguous()
    if spike:
        k[-1, :, seg - 3] = q[:Bkv, 0] * 4.0
    sk = _k_scales(k, H)
    sv = (v.float().abs().view(n_seg, Bkv, seg, H, HD).amax(dim=(0, 2, 4)) / 448.0).contiguous()
    segp = (seg + 63) // 64 * 64
    k8 = torch.empty(n_seg, *hip_lib.k8_shape(Bkv, H, seg), dtype=torch.uint8, device=DEV)
    vt8 = torch.empty(n_seg, Bkv, H, hip_lib.vt8_rows(HD), segp, dtype=torch.uint8, device=DEV)
    for s_ in range(n_seg):
        hip_lib.k_pack_fp8(k[s_], sk, k8[s_], H, HD)
        hip_lib.v_transpose_fp8(v[s_], sv, vt8[s_], H, HD)
    return q, k, v, sk, sv, k8, vt8, seg


def _run(hip_lib, q, k8, sk, vt8, sv, H, seg, n_seg, Bkv, workspace=False, lse=None, out=None):
    B, Lq, D = q.shape
    out = torch.empty(B, Lq, D, dtype=BF, device=DEV) if out is None else out
    ws = hip_lib.attention_workspace(q.device) if workspace else None
    hip_lib.attention_fwd_qk8(q, k8[0], sk, vt8, sv, out, H, HD, HD ** -0.5, seg_len=seg, lse=lse, n_seg=n_seg,
                              k_seg_stride=k8.stride(0), vt_seg_stride=vt8.stride(0), kv_batches=0 if Bkv == B else Bkv, workspace=ws)
    return out


def _qk8_case(hip_lib, B, H, Lq, Lk, n_seg=1, spike=False, workspace=False, Bkv=None, seed=220):
    Bkv = B if Bkv is None else Bkv
    D = H * HD
    q, k, v, sk, sv, k8, vt8, seg = _operands(hip_lib, B, H, Lq, Lk, n_seg, Bkv, spike, seed)
    lse = torch.empty(B, H, Lq, dtype=torch.float32, device=DEV)
    out = _run(hip_lib, q, k8, sk, vt8, sv, H, seg, n_seg, Bkv, workspace, lse)
    rep = lambda t: t.repeat(B // Bkv, 1, 1, 1)                                   # query batch b reads key batch b % Bkv
    heads = lambda t: t.permute(1, 0, 2, 3).reshape(Bkv, n_seg * seg, H, HD).permute(0, 2, 1, 3)   # [Bkv, H, Lk, hd]
    kk, vv = rep(heads(k).double()), rep(heads(v).float())
    sk_, sv_ = rep(sk[:, :, None, None]), rep(sv[:, :, None, None])
    # the kernel's operands, from the stated rules (f32 arithmetic, as on the device)
    k_q = ((heads(k).float() / sk[:, :, None, None]).clamp(-448, 448).to(F8).float() * sk[:, :, None, None])
    k_q = rep(k_q).double()
    v8 = ((vv / sv_).clamp(-448, 448).to(F8).float() * sv_).double()
    sc = torch.tensor(HD ** -0.5 * LOG2E, dtype=torch.float32).item()             # the kernel's f32 scale * log2(e)
    qf = q.float().view(B, Lq, H, HD).permute(0, 2, 1, 3) * sc
    amax = qf.abs().amax(-1, keepdim=True)
    sq = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    q_q = ((qf / sq).clamp(-448, 448).to(F8).float() * sq).double()               # log2 units
    qh = q.double().view(B, Lq, H, HD).permute(0, 2, 1, 3)
    s_ref = (qh @ kk.transpose(-1, -2)) * HD ** -0.5
    s_q = (q_q @ k_q.transpose(-1, -2)) / LOG2E                                   # natural-log units
    back = lambda o: o.permute(0, 2, 1, 3).reshape(B, Lq, D)
    ref = back(torch.softmax(s_ref, -1) @ vv.double())
    ref_q = back(torch.softmax(s_q, -1) @ v8)
    o = out.double()
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()
    r_kq, r_k, r_q = rel(o, ref_q), rel(o, ref), rel(ref_q, ref)
    d_lse = (lse.double() - torch.logsumexp(s_q, -1)).abs().max().item()
    print(f"qk8 B{B} H{H} Lq{Lq} Lk{Lk} seg{n_seg} Bkv{Bkv} spike{int(spike)} ws{int(workspace)}: rel(out,ref_q)={r_kq:.4e} "
          f"rel(out,ref)={r_k:.4e} rel(ref_q,ref)={r_q:.4e} dLSE={d_lse:.4e}")
    assert r_kq <= 4e-2, (r_kq, r_k, r_q)
    # the softmax denominator is the sum of the e4m3 P: a row dominated by one key carries that key's rounding, up to half an
    # e4m3 step (2^-4): ln(1 + 2^-4) = 0.061 (the argument of tests/test_gpu_fp8.py::_pv8_case)
    assert d_lse <= 7e-2, d_lse
    assert r_k <= r_q + 4e-2 + 1e-3, (r_k, r_q)
    return out


@pytest.mark.parametrize("Lq,Lk", [(256, 256), (300, 1000), (64, 65), (33, 704), (512, 4096)])
def test_attention_qk8_vs_f64(hip_lib, Lq, Lk):
    _qk8_case(hip_lib, 2, 2, Lq, Lk)


def test_attention_qk8_ragged_segments(hip_lib):
    _qk8_case(hip_lib, 2, 2, 130, 300, n_seg=3, seed=230)


def test_attention_qk8_reference_max_moves(hip_lib):
    """one key = 4 x a query row: the reference max moves by more than 2^8 and the rare path rescales O and the pending scores"""
    _qk8_case(hip_lib, 1, 2, 128, 900, spike=True, seed=231)


@pytest.mark.parametrize("B,H,Lq,Lk,n_seg", [(1, 17, 4096, 1000, 1), (2, 9, 4000, 400, 4)])
def test_attention_qk8_split_tail_units(hip_lib, B, H, Lq, Lk, n_seg):
    _qk8_case(hip_lib, B, H, Lq, Lk, n_seg=n_seg, workspace=True, seed=232)


def test_attention_qk8_shared_keys(hip_lib):
    _qk8_case(hip_lib, 4, 2, 200, 333, Bkv=2, seed=233)


def test_attention_qk8_constant_v_and_determinism(hip_lib):
    """V == c per channel: out == e4m3(c / s) * s whatever the scores are (the denominator is the ones row of the SAME fp8 product);
    12 runs bit-identical.  Pins the denominator and the epilogue."""
    B, H, Lq, Lk = 1, 8, 2000, 4133
    D = H * HD
    c = rnd("c", (D,), seed=243)
    q, k, v, sk, sv, k8, vt8, seg = _operands(hip_lib, B, H, Lq, Lk, 1, B, False, 241, const_v=c)
    outs = [_run(hip_lib, q, k8, sk, vt8, sv, H, seg, 1, B) for _ in range(12)]
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    c8 = (c.float().view(H, HD) / sv[0][:, None]).clamp(-448, 448).to(F8).float() * sv[0][:, None]
    assert (outs[0].float() - c8.view(1, 1, D)).abs().max().item() <= 2 ** -7 * c8.abs().max().item() + 1e-3


def test_attention_qk8_other_head_dims_are_unsupported(hip_lib):
    B, H, L, hd = 1, 2, 64, 72
    q = torch.zeros(B, L, H * hd, dtype=BF, device=DEV)
    k8 = torch.zeros(B, H, 64, 128, dtype=torch.uint8, device=DEV)
    vt8 = torch.zeros(B, H, hip_lib.vt8_rows(hd), 64, dtype=torch.uint8, device=DEV)
    s = torch.ones(B, H, dtype=torch.float32, device=DEV)
    out = torch.empty_like(q)
    st = torch.cuda.current_stream().cuda_stream
    rc = hip_lib.lib.osk_attention_fwd_qk8_bf16(q.data_ptr(), q.stride(0), q.stride(1), k8.data_ptr(), 0, k8.stride(0), 128, s.data_ptr(),
                                                vt8.data_ptr(), 0, s.data_ptr(), out.data_ptr(), out.stride(0), out.stride(1), None,
                                                B, H, L, 1, L, hd, hd ** -0.5, 0, 0, None, 0, st)
    assert rc == hip_lib.OSK_EUNSUPPORTED
    assert hip_lib.lib.osk_k_pack_fp8(q.data_ptr(), q.stride(0), q.stride(1), s.data_ptr(), k8.data_ptr(), B, L, H, hd, st) == hip_lib.OSK_EUNSUPPORTED


def test_attention_qk8_is_graph_capturable(hip_lib):
    """one call captured in a torch.cuda.graph and replayed twice == the eager result, bit for bit (default queue settings)"""
    B, H, Lq, Lk = 1, 2, 300, 333
    q, k, v, sk, sv, k8, vt8, seg = _operands(hip_lib, B, H, Lq, Lk, 1, B, False, 250)
    out = torch.empty(B, Lq, H * HD, dtype=BF, device=DEV)
    call = lambda: _run(hip_lib, q, k8, sk, vt8, sv, H, seg, 1, B, out=out)
    eager = call().clone()
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
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ------------------------------------------------------------------------------------------------ model gate (SURVEY.md 8(d), fp8 mode)
def test_mmdit_forward_fp8_mode_with_qk8(hip_lib):
    """MMDiTModel.enable_fp8(qk8=True) on the small head_dim-128 model of tests/test_gpu_fp8.py::test_mmdit_forward_fp8_mode: relL2 <= 5e-2
    against this package's bf16 path and against the fp32 oracle; the new entry is what runs; enable_fp8(False) restores bf16 bit-exactly."""
    from oracle import configs, mmdit_oracle as O
    from open_sora_amd import mmdit
    from tests.util import torch_inputs, torch_params

    cfg = dict(configs.GOLDEN["hd128_eager_fused"][0], depth=1, depth_single_blocks=1)
    geom = (2, 2, 12, 12, 160)
    model = mmdit.Flux(device_map="cuda", torch_dtype=BF, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=BF, device="cuda"), strict=True)
    inp = torch_inputs(cfg, *geom, dtype=BF, device="cuda")
    calls = []
    real = hip_lib.attention_fwd_qk8
    try:
        hip_lib.attention_fwd_qk8 = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        with torch.inference_mode():
            ref16 = model(**inp).clone()
            out_p8 = model.enable_fp8()(**inp).clone()
            assert not calls
            out8 = model.enable_fp8(qk8=True)(**inp).clone()
            n8 = len(calls)
            again16 = model.enable_fp8(False)(**inp).clone()
    finally:
        hip_lib.attention_fwd_qk8 = real
    assert n8 == 2 and len(calls) == 2
    assert torch.equal(again16, ref16)
    with torch.inference_mode():
        truth = O.forward(torch_params(cfg), cfg, **torch_inputs(cfg, *geom))
    rel = lambda a, b: ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm()).item()
    print(f"fp8 mode, small hd-128 model: qk8 vs bf16 {rel(out8, ref16):.4e}, qk8 vs fp32 {rel(out8, truth):.4e}; "
          f"pv8 vs bf16 {rel(out_p8, ref16):.4e}, pv8 vs fp32 {rel(out_p8, truth):.4e}")
    assert rel(out8, ref16) <= 5e-2 and rel(out8, truth) <= 5e-2, (rel(out8, ref16), rel(out8, truth))


def test_11b_shipped_shape_fp8_mode_with_qk8(hip_lib):
    """the same gate on the reference's shipped 11B geometry at its shipped shape (tests/golden/mmdit_fullsize_11b_d2s4.npz, depth
    2 + 4, 8,828 keys = 137 tiles + a ragged one), the way tests/test_gpu_baseline_geometry.py gates the pv8 fp8 mode on it"""
    import os

    import numpy as np

    from oracle import make_golden_fullsize_dit as FS
    from oracle import synth
    from tests.test_gpu_baseline_geometry import _to, _xl_model
    from tests.util import rel_l2

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mmdit_fullsize_11b_d2s4.npz"))
    cfg = FS.cfg_11b_d2s4()
    sd = {k: torch.from_numpy(v) for k, v in synth.make_params(synth.mmdit_param_shapes(cfg), 0, workers=min(16, os.cpu_count() or 1)).items()}
    model = _xl_model(cfg, sd)
    del sd
    G = FS.GEOM_11B
    inp = {k: torch.from_numpy(v) for k, v in synth.mmdit_inputs(cfg, 1, G["T"], G["h"], G["w"], G["L_txt"]).items()}
    truth = torch.from_numpy(g["out_s8"])
    res = {}
    for name, kw in (("pv8", {}), ("qk8", {"qk8": True})):
        model.enable_fp8(**kw)
        with torch.inference_mode():
            out8 = model(**_to(inp, BF, DEV)).float().cpu()
        assert torch.isfinite(out8).all()
        res[name] = rel_l2(torch.from_numpy(FS.summarize(out8[:1])["out_s8"]), truth)
    print(f"11B (depth 2 + 4) at the shipped 256 px shape, fp8 mode: lattice relL2 against the reference's fp32 truth: qk8 {res['qk8']:.3e}, "
          f"pv8 {res['pv8']:.3e} (gate 5e-2)")
    assert res["qk8"] <= 5e-2, res
