"""GPU: frame-window attention in fp8 mode (osk_attention_fwd_window_fp8_bf16).  (1) pv8 at head dims 72 / 128 and qk8 at 128,
a tile-aligned and a ragged body, shared and per-batch keys, tables from attention_window_table and hand-made ones (a 1-tile
interior run, a 2-tile run ending in the last tile, a run ending before it, the last tile alone), output and LSE per element against
the f64 reference on the e4m3 operands with the derived tolerance of tests/cpu_ops_window_fp8.py (the CPU suite shows that tolerance
rejecting a table off by one tile and a dropped prefix).  (2) The mask exactly, independent of that tolerance: with V the indicator
of a key's tile, an output dim IS the softmax mass a row put on that tile -- exactly zero outside the row's key set.  (3) Full
ranges without a prefix bit for bit the unwindowed fp8 entries.  (4) Refused arguments.  (5) A two-block fp8 MMDiT with the window
on against the same forward on the CPU statement.  (6) The sampler's loop under hip_graph=True bit for bit the eager one.  Each
check prints its figures before it asserts."""
import pytest
import torch

from oracle import sampling_oracle as S
from tests import cpu_ops_window_fp8 as F
from tests.test_attention_window_fp8_host import MODELS, _N, _T, _h, _w, _LT, build, cpu_forwards, model_case, packed
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
R = F.R
H_, B_, NP, LQ = F.H_, F.B_, F.NP, F.LQ


def _run(hip_lib, q, ops, hd, kind, table, n_prefix, Bkv, Lk, lse=True):
    kk, sk, vt8, sv = ops
    out = torch.full_like(q, float("nan"))
    l = torch.full((q.shape[0], H_, q.shape[1]), float("nan"), device=DEV) if lse else None
    hip_lib.attention_fwd_window_fp8(q, kk, sk, vt8, sv, out, H_, hd, hd ** -0.5, n_prefix=n_prefix, windows=table, mode=kind, lse=l,
                                     q_prescaled=True, kv_batches=0 if Bkv == q.shape[0] else Bkv, Lk=Lk)
    torch.cuda.synchronize()
    return out.cpu(), None if l is None else l.cpu()


# ----------------------------------------------------------------------------- 1. per element vs f64
@pytest.mark.parametrize("Bkv", [1, 2])
@pytest.mark.parametrize("body", F.BODIES)
@pytest.mark.parametrize("kind,hd", F.KIND_HD)
def test_fp8_window_entry_vs_f64(hip_lib, kind, hd, body, Bkv):
    worst = 0.0
    for table in F.TABLES:
        q, k, v, t, ref = F.case(kind, hd, body, Bkv, table)
        ops = packed(hip_lib, k, v, hd, kind, DEV)
        out, lse = _run(hip_lib, q.to(DEV), ops, hd, kind, t, NP, Bkv, k.shape[1])
        finite = bool(torch.isfinite(out.float()).all() and torch.isfinite(lse).all())
        r = R.ratios(R.heads(out.float(), H_, hd), lse, ref)
        print(f"fp8 window {kind} hd {hd} body {body} Bkv {Bkv} {table}: finite {finite}  err/tol {r[0]:.3f}  dlse/tol {r[1]:.3f}")
        assert finite
        worst = max(worst, *r)
    assert worst <= 1.0, worst


# ----------------------------------------------------------------------------- 2. the mask, exactly
@pytest.mark.parametrize("body", F.BODIES)
@pytest.mark.parametrize("kind,hd", F.KIND_HD)
def test_tile_indicator_values_show_the_mask_exactly(hip_lib, kind, hd, body):
    """V[key, d] = 1 where key lies in body tile d (d < 8), V[key, 9] = 1 for a prefix key, 0 elsewhere: every value, and the scale
    1 / 448, is exact in e4m3, so out[row, d] is the share of the row's softmax mass on tile d (dim 9: on the prefix) and a tile the
    row must not see contributes no term at all -- exactly 0.  Scores are diffuse (below 1 log2 unit in magnitude, so every P lies
    in [1/4, 1] and carries e4m3's relative error of 2^-4 only): a visible tile's share is within a few percent of the f64 share,
    and 'at least half' cannot fail for any reason but the mask."""
    Lk, tiles = NP + body, (body + 63) // 64
    g = torch.Generator().manual_seed(31 * hd + body)
    k = torch.randn(B_, Lk, H_ * hd, generator=g).to(BF)
    q = torch.randn(B_, LQ, H_ * hd, generator=g)
    kn = k.float().reshape(B_, Lk, H_, hd).norm(dim=-1).max()
    q = (q * (0.9 / float(q.reshape(B_, LQ, H_, hd).norm(dim=-1).max() * kn))).to(BF)     # |q . k| <= |q| |k| <= 0.9 log2 units
    v = torch.zeros(B_, Lk, H_, hd)
    v[:, :NP, :, 9] = 1.0
    for j in range(tiles):
        v[:, NP + 64 * j: NP + 64 * (j + 1), :, j] = 1.0
    v = v.reshape(B_, Lk, H_ * hd).to(BF)
    ops = packed(hip_lib, k, v, hd, kind, DEV)
    assert bool((ops[3] == 1.0 / 448.0).all())
    qm, km, _, _, _ = F.mfma_operands(q, k, v, H_, hd, kind)
    s = qm.double() @ km.double().transpose(-1, -2)                                        # [B, H, LQ, Lk]
    assert float(s.abs().max()) < 1.0
    for table in F.TABLES:
        t = F.make_table(table, NP, body)
        out, _ = _run(hip_lib, q.to(DEV), ops, hd, kind, t, NP, B_, Lk, lse=False)
        o = R.heads(out.float(), H_, hd).double()
        lo = 1.0
        for i, (first, n) in enumerate(t.tolist()):
            rows = slice(256 * i, min(256 * (i + 1), LQ))
            keys = F.block_keys(NP, Lk, first, n)
            p = torch.softmax(s[:, :, rows][..., keys] * R.LN2, -1)
            inside = [9] + list(range(first, first + n))
            outside = [d for d in range(hd) if d not in inside]
            stray = o[:, :, rows][..., outside].abs().max().item()
            print(f"tile indicator {kind} hd {hd} body {body} {table} block {i} ({first}, {n}): largest value outside the key set {stray:.3e}")
            assert stray == 0.0, (table, i, stray)
            for d in inside:
                sel = keys < NP if d == 9 else (keys >= NP + 64 * d) & (keys < NP + 64 * (d + 1))
                mass = p[..., sel].sum(-1)
                lo = min(lo, (o[:, :, rows, d] / mass).min().item())
        print(f"tile indicator {kind} hd {hd} body {body} {table}: smallest (kernel mass / f64 mass) inside the key sets {lo:.3f}")
        assert lo >= 0.5, (table, lo)


# ----------------------------------------------------------------------------- 3. full ranges, no prefix: the unwindowed entries
@pytest.mark.parametrize("kind,hd", F.KIND_HD)
def test_full_ranges_without_a_prefix_are_the_unwindowed_entry_bit_for_bit(hip_lib, kind, hd):
    Lk = NP + 484                                                                          # 9 tiles, the last one ragged
    q, k, v = F.operands_fp8(hd, H_, B_, 2, LQ, Lk)
    qd = q.to(DEV)
    ops = packed(hip_lib, k, v, hd, kind, DEV)
    kk, sk, vt8, sv = ops
    out, lse = _run(hip_lib, qd, ops, hd, kind, torch.tensor([[0, 9]] * 4, dtype=torch.int32), 0, 2, Lk)
    want, want_lse = torch.full_like(qd, float("nan")), torch.full((B_, H_, LQ), float("nan"), device=DEV)
    if kind == "qk8":
        hip_lib.attention_fwd_qk8(qd, kk, sk, vt8, sv, want, H_, hd, hd ** -0.5, seg_len=Lk, lse=want_lse, q_prescaled=True)
    else:
        hip_lib.attention_fwd_pv8(qd, kk, vt8, sv, want, H_, hd, hd ** -0.5, lse=want_lse, q_prescaled=True)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out.view(torch.int16), want.cpu().view(torch.int16)) and torch.equal(lse, want_lse.cpu())


# ----------------------------------------------------------------------------- 4. refused arguments
def test_refused_arguments(hip_lib):
    """status codes of the entry, below the binding's own checks: nothing is launched"""
    hd, Lq, Lk = 128, 800, 512
    q = torch.zeros(1, Lq, H_ * hd, dtype=BF, device=DEV)
    k = torch.zeros(1, Lk, H_ * hd, dtype=BF, device=DEV)
    k8 = torch.zeros(1, H_, Lk, 128, dtype=torch.uint8, device=DEV)
    vt8 = torch.zeros(1, H_, 144, Lk, dtype=torch.uint8, device=DEV)
    vt8[:, :, hd] = 0x38                                      # the validity / denominator row: 1.0 in e4m3 for every key
    sc = torch.ones(2, H_, device=DEV)                        # row 0: k_scale, row 1: v_scale
    out = torch.full_like(q, 3.0)
    win = torch.tensor([[0, 7]] * 4, dtype=torch.int32, device=DEV)
    ws = hip_lib.attention_window_workspace(1, H_, Lq, 128, DEV)
    EINVAL, EUNSUP = -1, hip_lib.OSK_EUNSUPPORTED
    PV8, QK8 = hip_lib.ATTN_MODES["pv8"], hip_lib.ATTN_MODES["qk8"]

    def call(mode=PV8, n_prefix=64, n_windows=4, table=win.data_ptr(), workspace=ws.data_ptr(), ws_bytes=ws.numel(), hd_=hd, kbs=None,
             krs=None, k_scale=sc[0].data_ptr(), v_scale=sc[1].data_ptr()):
        kt = k8 if mode == QK8 else k
        return hip_lib.lib.osk_attention_fwd_window_fp8_bf16(
            q.data_ptr(), q.stride(0), q.stride(1), kt.data_ptr(), kt.stride(0) if kbs is None else kbs,
            (128 if mode == QK8 else kt.stride(1)) if krs is None else krs, k_scale, vt8.data_ptr(), v_scale, out.data_ptr(),
            out.stride(0), out.stride(1), None, 1, H_, Lq, Lk, n_prefix, hd_, 0.125, 1, 0, mode, table, n_windows, workspace, ws_bytes,
            torch.cuda.current_stream().cuda_stream)

    for mode in (PV8, QK8):
        # the bf16 entry's list
        assert call(mode, n_windows=3) == EINVAL and call(mode, n_windows=5) == EINVAL
        assert call(mode, table=None) == EINVAL and call(mode, table=win.data_ptr() + 2) == EINVAL
        assert call(mode, n_prefix=32) == EINVAL and call(mode, n_prefix=Lk) == EINVAL and call(mode, n_prefix=-64) == EINVAL
        assert call(mode, workspace=None, ws_bytes=0) == EINVAL and call(mode, ws_bytes=1024) == EINVAL
        # the scales
        assert call(mode, v_scale=None) == EINVAL and call(mode, v_scale=sc[1].data_ptr() + 2) == EINVAL
        assert call(mode, hd_=96) == EUNSUP and call(mode, hd_=64) == EUNSUP
    assert call(0) == EINVAL and call(3) == EINVAL            # OSK_ATTN_BF16 = 0 (the bf16 entry's business), and no mode at all
    assert call(QK8, k_scale=None) == EINVAL and call(QK8, k_scale=sc[0].data_ptr() + 2) == EINVAL
    assert call(QK8, kbs=k8.stride(0) + 8) == EINVAL and call(QK8, kbs=-k8.stride(0)) == EINVAL
    assert call(QK8, krs=256) == EUNSUP and call(QK8, hd_=72) == EUNSUP
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    # good calls: zero K and V -- uniform probabilities over zero values, so every output is exactly 0 where it was 3.0
    for good in (dict(mode=PV8, k_scale=None), dict(mode=QK8)):      # (pv8 ignores k_scale)
        out.fill_(3.0)
        assert call(**good) == 0
        torch.cuda.synchronize()
        assert bool((out == 0.0).all())


# ----------------------------------------------------------------------------- 5. end to end
@pytest.mark.parametrize("hd", [72, 128])
def test_windowed_fp8_mmdit_matches_the_cpu_statement(hip_lib, hd):
    """one double and one single block in fp8 mode (head_dim 72: pv8; 128: qk8), window 0, QK-norm scales raised so that attention
    is peaked.  e_off: HIP vs CPU fp8 forward with the window off -- the noise floor; e_win: the same with the window on; sep: the
    distance between the two CPU forwards (no GPU in it; tests/test_attention_window_fp8_host.py holds it to >= 0.2).  The windowed
    HIP forward has to pass the project's fp8 gate (5e-2), lie nearer than sep / 2 to the windowed CPU forward and farther than
    sep / 2 from the unwindowed one; the comparison means something only where sep >= 4 e_off."""
    from open_sora_amd import mmdit

    x = {k_: v_.to(DEV) for k_, v_ in model_case(hd)[2].items()}
    model = build(mmdit, hd, DEV)
    with torch.inference_mode():
        got = model.set_attention_window(0, _N)(**x).float().cpu()
        rep = model.attention_report()["attention_window"]
        off = model.set_attention_window(None)(**x).float().cpu()
    mmdit.set_ops_for_testing(F)
    try:
        want, full = cpu_forwards(hd)
    finally:
        mmdit.set_ops_for_testing(hip_lib)
    e_off, e_win, sep, e_full = rel_l2(off, full), rel_l2(got, want), rel_l2(want, full), rel_l2(got, full)
    print(f"fp8 windowed MMDiT hd {hd} {MODELS[hd][1]}: e_off {e_off:.3e}  e_win {e_win:.3e}  sep {sep:.3e}  windowed HIP vs unwindowed CPU {e_full:.3e}")
    assert rep["mode"] == MODELS[hd][1] and rep["window_frames"] == 0
    assert torch.isfinite(got).all() and sep >= 4 * e_off, "the condition of the comparison"
    assert e_win <= 5e-2 and e_win <= sep / 2 and e_full > sep / 2


# ----------------------------------------------------------------------------- 6. hipGraph
def test_windowed_fp8_loop_under_hipgraph_is_the_eager_loop(hip_lib):
    from open_sora_amd import mmdit, sampling

    cfg = model_case(128)[0]
    n, T, Hh, Ww, Lt = 1, _T, 2 * _h, 2 * _w, _LT
    g = torch.Generator().manual_seed(11)
    z = torch.randn(n, 16, T, Hh, Ww, generator=g).bfloat16().float()
    masks = torch.zeros(n, 1, T, Hh, Ww)
    masks[:, :, 0] = 1
    masked_ref = (torch.randn(n, 16, T, Hh, Ww, generator=g) * masks).bfloat16().float()
    txt = (torch.randn(3 * n, Lt, cfg["context_in_dim"], generator=g) * 0.2).bfloat16().float()
    y_vec = torch.randn(3 * n, cfg["vec_in_dim"], generator=g).bfloat16().float()
    img_ids, txt_ids = S.grid_ids(3 * n, T, Hh // 2, Ww // 2, Lt, torch.float32)
    tensors = dict(img=S.pack(z).repeat(3, 1, 1), masks=masks, masked_ref=masked_ref, img_ids=img_ids, txt=txt, txt_ids=txt_ids, y_vec=y_vec)
    args = dict({k_: v_.to(DEV, BF) for k_, v_ in tensors.items()}, timesteps=sampling.get_schedule(4, 96, T), guidance=7.5, guidance_img=3.0)
    model = build(mmdit, 128, DEV).set_attention_window(3, _N)     # enable_fp8(qk8=True); a setting of the model's own
    with torch.inference_mode():
        plain = sampling.I2VDenoiser().denoise(model.set_attention_window(None), **dict(args))
        model.set_attention_window(3, _N)
        eager = sampling.I2VDenoiser().denoise(model, attn_window_frames=1, **dict(args))
        graphed = sampling.I2VDenoiser().denoise(model, attn_window_frames=1, hip_graph=True, **dict(args))
        torch.cuda.synchronize()
    assert model._attn_window == (3, _N), "the model's own window setting was not restored"
    assert model.attention_report()["attention_window"]["mode"] == "qk8"
    assert torch.isfinite(eager.float()).all() and not torch.equal(eager, plain)
    assert torch.equal(eager, graphed), "the replayed windowed fp8 loop differs from the eager one"
