"""GPU: frame-window attention.  (1) osk_attention_fwd_window_bf16 at head dims 64 / 72 / 128, FAST and general body, shared and
per-batch keys, a tile-aligned and a ragged body, tables from attention_window_table and a hand-made one (1-tile and 2-tile ranges,
a range that ends in the ragged tile and one that ends before it), output and LSE per element against the f64 reference and derived
tolerance of tests/cpu_ops_window.py (the CPU suite shows that tolerance rejecting a table off by one tile and a dropped prefix);
full ranges without a prefix bit for bit osk_attention_fwd_bf16; full ranges with a prefix within the merge tolerance of the full
call; refused arguments.  (2) a two-block MMDiT with the window on against the same forward on the CPU statement of the entry,
and the sampler's loop under hip_graph=True bit for bit the eager one.  Each check prints its figures before it asserts."""
import pytest
import torch

from oracle import configs, sampling_oracle as S
from tests import cpu_ops_window as W
from tests.test_attention_window_host import B_, H_, case
from tests.test_gpu_mmdit import _build
from tests.util import rel_l2, torch_inputs, torch_params

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
R = W.R
NP = 64


def _vt(hip_lib, v, hd):
    Bkv, L, _ = v.shape
    vt = torch.zeros(Bkv, H_, hd, (L + 63) // 64 * 64, dtype=BF, device=DEV)
    hip_lib.v_transpose(v, vt, H_, hd)
    return vt


def _run(hip_lib, q, k, vt, hd, table, n_prefix, bound, Bkv):
    out = torch.full_like(q, float("nan"))
    lse = torch.full((q.shape[0], H_, q.shape[1]), float("nan"), device=DEV)
    hip_lib.attention_fwd_window(q, k, vt, out, H_, hd, hd ** -0.5, n_prefix=n_prefix, windows=table, lse=lse, q_prescaled=True,
                                 kv_batches=0 if Bkv == q.shape[0] else Bkv, score_bound=bound)
    torch.cuda.synchronize()
    return out.cpu(), lse.cpu()


@pytest.mark.parametrize("Bkv", [1, 2])
@pytest.mark.parametrize("body", [960, 996])
@pytest.mark.parametrize("hd", [64, 72, 128])
def test_window_entry_vs_f64(hip_lib, hd, body, Bkv):
    worst = 0.0
    for table in ("w0", "w1", "hand"):
        q, k, v, sb, t, ref = case(hd, body, Bkv, table)
        qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
        vt = _vt(hip_lib, vd, hd)
        for bound in (sb, 0.0):
            assert hip_lib.attention_body(hd, 1, body, bound).endswith("<FAST>" if bound else "<general>")
            out, lse = _run(hip_lib, qd, kd, vt, hd, t, NP, bound, Bkv)
            assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
            r = R.ratios(R.heads(out.float(), H_, hd), lse, ref)
            print(f"window hd {hd} body {body} Bkv {Bkv} {table} {'FAST' if bound else 'general'}: err/tol {r[0]:.3f}  dlse/tol {r[1]:.3f}")
            worst = max(worst, *r)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("hd", [64, 72, 128])
def test_full_ranges_without_a_prefix_are_the_plain_call_bit_for_bit(hip_lib, hd):
    q, k, v, sb = W.operands(hd, H_, B_, 2, 1060)                 # 17 tiles, the last one ragged; 5 query blocks, the last partial
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    vt = _vt(hip_lib, vd, hd)
    t = torch.tensor([[0, 17]] * 5, dtype=torch.int32)
    out, lse = _run(hip_lib, qd, kd, vt, hd, t, 0, 0.0, 2)
    want, want_lse = torch.full_like(qd, float("nan")), torch.full((B_, H_, 1060), float("nan"), device=DEV)
    hip_lib.attention_fwd(qd, kd, vt, want, H_, hd, hd ** -0.5, lse=want_lse, q_prescaled=True)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), want.cpu().view(torch.int16)) and torch.equal(lse, want_lse.cpu())


@pytest.mark.parametrize("hd", [64, 72, 128])
def test_full_ranges_with_a_prefix_agree_with_the_full_call(hip_lib, hd):
    q, k, v, sb, t, ref = case(hd, 996, 2, "w12")
    assert t.tolist() == [[0, 16]] * 5
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    vt = _vt(hip_lib, vd, hd)
    full_ref = R.reference(R.mfma_q(q, H_, hd, 1.0, True, "bf16"), R.mfma_k(k[None], H_, hd, "bf16"), R.mfma_v(v[None], H_, hd, "bf16"), "bf16")
    for bound in (sb, 0.0):
        out, lse = _run(hip_lib, qd, kd, vt, hd, t, NP, bound, 2)
        want, want_lse = torch.full_like(qd, float("nan")), torch.full((B_, H_, 1060), float("nan"), device=DEV)
        hip_lib.attention_fwd(qd, kd, vt, want, H_, hd, hd ** -0.5, lse=want_lse, q_prescaled=True, score_bound=bound)
        torch.cuda.synchronize()
        r_win = R.ratios(R.heads(out.float(), H_, hd), lse, ref)
        r_full = R.ratios(R.heads(want.cpu().float(), H_, hd), want_lse.cpu(), full_ref)
        d = (R.heads(out.float(), H_, hd).double() - R.heads(want.cpu().float(), H_, hd).double()).abs() / (ref["tol"] + full_ref["tol"])
        print(f"W = T hd {hd} {'FAST' if bound else 'general'}: windowed err/tol {r_win[0]:.3f}, full call {r_full[0]:.3f}, |windowed - full| / (tol + tol) {d.max():.3f}")
        assert max(r_win) <= 1.0 and max(r_full) <= 1.0 and d.max() <= 1.0


def test_refused_arguments(hip_lib):
    """status codes of the entry, below the binding's own checks: nothing is launched"""
    hd, L = 64, 1024
    q = torch.zeros(1, L, H_ * hd, dtype=BF, device=DEV)
    vt = torch.zeros(1, H_, hd, L, dtype=BF, device=DEV)
    out = torch.full_like(q, 3.0)
    win = torch.tensor([[0, 15]] * 4, dtype=torch.int32, device=DEV)
    ws = hip_lib.attention_window_workspace(1, H_, L, 128, DEV)
    EINVAL = -1

    def call(n_prefix=64, n_windows=4, table=win.data_ptr(), workspace=ws.data_ptr(), ws_bytes=ws.numel(), bound=0.0, hd_=hd):
        return hip_lib.lib.osk_attention_fwd_window_bf16(q.data_ptr(), q.stride(0), q.stride(1), q.data_ptr(), q.stride(0), q.stride(1),
                                                         vt.data_ptr(), out.data_ptr(), out.stride(0), out.stride(1), None, 1, H_, L, L,
                                                         n_prefix, hd_, 0.125, 1, 0, bound, table, n_windows, workspace, ws_bytes,
                                                         torch.cuda.current_stream().cuda_stream)

    assert call(n_windows=3) == EINVAL and call(n_windows=5) == EINVAL
    assert call(table=None) == EINVAL and call(table=win.data_ptr() + 2) == EINVAL
    assert call(n_prefix=32) == EINVAL and call(n_prefix=L) == EINVAL and call(n_prefix=-64) == EINVAL
    assert call(workspace=None, ws_bytes=0) == EINVAL and call(ws_bytes=1024) == EINVAL
    assert call(bound=-1.0) == EINVAL and call(bound=float("nan")) == EINVAL
    assert call(hd_=96) == hip_lib.OSK_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    assert call() == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- end to end
_T, _h, _w, _LT = 6, 8, 12, 64                              # 64 text + 6 frames x 96 image tokens


def test_windowed_mmdit_matches_the_cpu_statement(hip_lib):
    """one double block and one single block, window 1: the HIP forward against the same forward on tests/cpu_ops_window.py.  Both
    are bf16 pipelines over the same roundings in another summation order; a tensor rounded to bf16 differs by at most one unit in
    the last place (2^-8 relative) where the f32 values straddle a tie, and about a dozen rounded tensors lie between input and
    output of two blocks: relL2 <= sqrt(12) 2^-9 ~ 0.007 if every one of them differed everywhere; the bound is 2^-7.  The mask
    must be felt as well.  With sep the distance between the windowed and the unwindowed CPU forward (no GPU in it), a forward
    that ignored the mask would lie about sep from the windowed one: the result has to be nearer than sep / 2 to the windowed
    forward and farther than sep / 2 from the unwindowed one.  (Synthetic weights attend diffusely: sep is about 1e-2.)"""
    from open_sora_amd import mmdit

    cfg = dict(configs.GOLDEN["hd72_eager_split"][0], depth=1, depth_single_blocks=1)
    x = torch_inputs(cfg, 1, _T, _h, _w, _LT, dtype=BF)
    model = _build(cfg).set_attention_window(1, _h * _w)
    with torch.inference_mode():
        got = model(**{k_: v_.to(DEV) for k_, v_ in x.items()}).float().cpu()
        off = model.set_attention_window(None)(**{k_: v_.to(DEV) for k_, v_ in x.items()}).float().cpu()
    rep = model.set_attention_window(1, _h * _w).attention_report()
    assert rep["attention_window"]["window_frames"] == 1
    mmdit.set_ops_for_testing(W)
    try:
        cpu = mmdit.Flux(device_map="cpu", torch_dtype=BF, **cfg)
        cpu.load_state_dict(torch_params(cfg, dtype=BF), strict=True)
        with torch.inference_mode():
            want = cpu.set_attention_window(1, _h * _w)(**x).float()
            full = cpu.set_attention_window(None)(**x).float()
    finally:
        mmdit.set_ops_for_testing(hip_lib)
    e_win, e_full, e_off, sep = rel_l2(got, want), rel_l2(got, full), rel_l2(off, full), rel_l2(full, want)
    print(f"windowed MMDiT: relL2 vs the windowed CPU forward {e_win:.3e}, vs the unwindowed one {e_full:.3e}; window off vs unwindowed "
          f"{e_off:.3e}; the two CPU forwards are {sep:.3e} apart")
    assert torch.isfinite(got).all() and e_win <= min(2.0 ** -7, sep / 2) and e_off <= 2.0 ** -7 and e_full >= sep / 2


def test_windowed_loop_under_hipgraph_is_the_eager_loop(hip_lib):
    from open_sora_amd import sampling

    cfg = dict(configs.GOLDEN["hd72_eager_split"][0], depth=1, depth_single_blocks=1)
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
    model = _build(cfg)
    with torch.inference_mode():
        plain = sampling.I2VDenoiser().denoise(model, **dict(args))
        eager = sampling.I2VDenoiser().denoise(model, attn_window_frames=1, **dict(args))
        graphed = sampling.I2VDenoiser().denoise(model, attn_window_frames=1, hip_graph=True, **dict(args))
        pruned = sampling.I2VDenoiser().denoise(model, attn_window_frames=1, hip_graph=True, cfg_prune=True, **dict(args))
        torch.cuda.synchronize()
    assert model._attn_window is None
    assert torch.isfinite(eager.float()).all() and not torch.equal(eager, plain)
    assert torch.equal(eager, graphed), "the replayed windowed loop differs from the eager one"
    assert torch.isfinite(pruned.float()).all()
