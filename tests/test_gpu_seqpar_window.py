"""GPU: frame-window attention under sequence parallelism.
1. osk_kv_join_bf16 bit for bit: vt_out == osk_v_transpose_bf16 of the de-segmented V, k_out == the de-segmented K; head_dim 64 / 72 /
   128, tile-misaligned segments and a short last segment, L % 64 zero and non-zero, inputs inside a larger strided buffer, outputs
   (k_out a strided view) inside guard bands; every refused argument returns its code and leaves the outputs untouched.
2. join + window call captured in a torch.cuda.graph and replayed == the eager pair.
3. one rank's join -> window path, P = 2 (L = 640, Lc = 320) and P = 3 (ragged: 214, 214, 212), W = 1, head_dim 72 / 128: output and LSE
   per element against the f64 reference over each block's stated key set, with the derived tolerance of tests/cpu_ops_window.py
   (which the CPU suite shows rejecting a table off by one tile: mass outside the stated keys leaves it).
4. the model with P ranks as threads (tests/local_transport.py), both exchange modes: an aligned split against the single-device
   windowed forward, unaligned and ragged splits with full tables against the sharded forward without a window (2^-7, the bound
   tests/test_gpu_seqpar_ragged.py holds a sharded forward to against the single device), and the launches with the window off.
Each check prints its figures before it asserts."""
import functools

import pytest
import torch

from tests import cpu_ops_window as W
from tests.test_gpu_seqpar_ragged import _Counting, _guarded, _guards_intact, _ranks_forward
from tests.util import rel_l2, torch_inputs, torch_params

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
R = W.R
EINVAL = -1


def _segments(x, n_seg, seg_len, pad_rows=3, pad_cols=16, fill=float("nan")):
    """x [B, L, D] cut into n_seg segments of seg_len rows (the last one short) inside a larger strided buffer [n_seg, B, seg_len +
    pad_rows, D + pad_cols]; everything that is not a key -- pad rows, pad columns, the rows behind the last key -- holds `fill`"""
    B, L, D = x.shape
    wide = torch.full((n_seg, B, seg_len + pad_rows, D + pad_cols), fill, dtype=x.dtype, device=x.device)
    seg = wide[:, :, :seg_len, pad_cols // 2: pad_cols // 2 + D]
    for s in range(n_seg):
        rows = x[:, s * seg_len: min((s + 1) * seg_len, L)]
        seg[s, :, :rows.shape[1]] = rows
    return seg


# ----------------------------------------------------------------------------- 1. the join
@pytest.mark.parametrize("n_seg,seg_len,L", [(3, 100, 237), (2, 64, 128), (4, 33, 130)])
@pytest.mark.parametrize("hd", [64, 72, 128])
def test_join_is_bit_exact(hip_lib, hd, n_seg, seg_len, L):
    B, H = 2, 2
    D, Lp = H * hd, (L + 63) // 64 * 64
    g = torch.Generator(device=DEV).manual_seed(hd + L)
    k = torch.randn(B, L, D, device=DEV, generator=g).to(BF)
    v = torch.randn(B, L, D, device=DEV, generator=g).to(BF)
    k_seg, v_seg = _segments(k, n_seg, seg_len), _segments(v, n_seg, seg_len)
    ko_raw, ko_wide, ko_pad = _guarded((B, L, D + 8), BF)
    k_out = ko_wide[:, :, :D]                                   # a view with strides of its own
    vt_raw, vt_out, vt_pad = _guarded((B, H, hd, Lp), BF)
    hip_lib.kv_join(k_seg, v_seg, k_out, vt_out, H, hd, L)
    want = torch.full((B, H, hd, Lp), 3.0, dtype=BF, device=DEV)
    hip_lib.v_transpose(v, want, H, hd)
    torch.cuda.synchronize()
    assert _guards_intact(ko_raw, ko_pad) and _guards_intact(vt_raw, vt_pad)
    assert bool((ko_wide[:, :, D:].view(torch.uint8) == 0xA5).all()), "the columns beside k_out were written"
    assert torch.equal(vt_out.view(torch.int16), want.view(torch.int16))
    assert torch.equal(k_out.view(torch.int16), k.view(torch.int16))


def test_join_status_codes(hip_lib):
    """every refused call returns its code and launches nothing: the outputs keep their fill"""
    B, H, hd, n_seg, seg_len, L = 1, 2, 64, 3, 100, 237
    D = H * hd
    k_seg = torch.zeros(n_seg, B, seg_len, D, dtype=BF, device=DEV)
    k_out = torch.full((B, L, D), 3.0, dtype=BF, device=DEV)
    vt_out = torch.full((B, H, hd, 256), 3.0, dtype=BF, device=DEV)

    def call(k=k_seg.data_ptr(), v=k_seg.data_ptr(), ss=k_seg.stride(0), bs=k_seg.stride(1), rs=k_seg.stride(2), ko=k_out.data_ptr(),
             kobs=k_out.stride(0), kors=k_out.stride(1), vt=vt_out.data_ptr(), B_=B, H_=H, hd_=hd, n=n_seg, sl=seg_len, L_=L):
        return hip_lib.lib.osk_kv_join_bf16(k, v, ss, bs, rs, ko, kobs, kors, vt, B_, H_, hd_, n, sl, L_, torch.cuda.current_stream().cuda_stream)

    bad = [dict(L_=0), dict(L_=200), dict(L_=301), dict(n=0), dict(n=2), dict(n=4), dict(sl=0), dict(sl=78), dict(sl=119), dict(B_=0), dict(H_=0),
           dict(k=None), dict(v=None), dict(ko=None), dict(vt=None),
           dict(k=k_seg.data_ptr() + 2), dict(v=k_seg.data_ptr() + 8), dict(ko=k_out.data_ptr() + 4), dict(vt=vt_out.data_ptr() + 2),
           dict(ss=k_seg.stride(0) + 4), dict(bs=k_seg.stride(1) + 1), dict(rs=D + 4), dict(kobs=k_out.stride(0) + 2), dict(kors=D + 4)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
    for hd_ in (96, 32, 256):
        assert call(hd_=hd_) == hip_lib.OSK_EUNSUPPORTED, hd_
    torch.cuda.synchronize()
    assert bool((k_out == 3.0).all()) and bool((vt_out == 3.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((k_out == 0).all()) and bool((vt_out[..., :L] == 0).all())


# ----------------------------------------------------------------------------- 3. one rank's join -> window path vs f64
H_, B_ = 2, 2
_LT, _N, _T = 64, 96, 6
_L = _LT + _N * _T                                              # 640


@functools.lru_cache(maxsize=None)
def _rank_case(hd: int, P: int):
    """operands of the whole sequence and, per rank, (row0, rows, table, f64 reference over each block's stated keys): computed once"""
    from open_sora_amd.mmdit import attention_window_table

    q, k, v, sb = W.operands(hd, H_, B_, B_, _L)
    Lc = -(-_L // P)
    ranks = []
    for r in range(P):
        row0, rows = r * Lc, min((r + 1) * Lc, _L) - r * Lc
        t = attention_window_table(_LT, _N * _T, _N, 1, row0=row0, n_rows=rows)
        ranks.append((row0, rows, t, W.reference(q[:, row0: row0 + rows].contiguous(), k, v, H_, hd, _LT, t)))
    return q, k, v, sb, Lc, ranks


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("hd", [72, 128])
def test_rank_join_then_window_vs_f64(hip_lib, hd, P):
    q, k, v, sb, Lc, ranks = _rank_case(hd, P)
    assert (Lc, ranks[-1][1]) == ((320, 320) if P == 2 else (214, 212))
    assert any(t[:, 1].max() < (_N * _T + 63) // 64 for _, _, t, _ in ranks), "no block with a real window"
    qd = q.to(DEV)
    k_seg, v_seg = _segments(k.to(DEV), P, Lc, fill=100.0), _segments(v.to(DEV), P, Lc, fill=100.0)
    D, Lp = H_ * hd, (_L + 63) // 64 * 64
    kj = torch.empty(B_, _L, D, dtype=BF, device=DEV)
    vtj = torch.empty(B_, H_, hd, Lp, dtype=BF, device=DEV)
    hip_lib.kv_join(k_seg, v_seg, kj, vtj, H_, hd, _L)
    worst = 0.0
    for rank, (row0, rows, t, ref) in enumerate(ranks):
        for bound in (sb, 0.0):
            qr = qd[:, row0: row0 + rows]
            out = torch.full((B_, rows, D), float("nan"), dtype=BF, device=DEV)
            lse = torch.full((B_, H_, rows), float("nan"), device=DEV)
            hip_lib.attention_fwd_window(qr, kj, vtj, out, H_, hd, hd ** -0.5, n_prefix=_LT, windows=t, lse=lse, q_prescaled=True, score_bound=bound)
            torch.cuda.synchronize()
            out, lse = out.cpu(), lse.cpu()
            assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
            r = R.ratios(R.heads(out.float(), H_, hd), lse, ref)
            print(f"join -> window hd {hd} P {P} rank {rank} rows [{row0}, {row0 + rows}) table {t.tolist()} {'FAST' if bound else 'general'}: "
                  f"err/tol {r[0]:.3f}  dlse/tol {r[1]:.3f}")
            worst = max(worst, *r)
    assert worst <= 1.0, worst


# ----------------------------------------------------------------------------- 2. capture
def test_join_and_window_call_replay_from_a_graph(hip_lib):
    hd, P = 72, 3
    q, k, v, sb, Lc, ranks = _rank_case(hd, P)
    row0, rows, t, _ = ranks[1]
    D, Lp = H_ * hd, (_L + 63) // 64 * 64
    k_seg, v_seg = torch.zeros(P, B_, Lc, D, dtype=BF, device=DEV), torch.zeros(P, B_, Lc, D, dtype=BF, device=DEV)
    qr = torch.empty(B_, rows, D, dtype=BF, device=DEV)
    kj, vtj = torch.empty(B_, _L, D, dtype=BF, device=DEV), torch.empty(B_, H_, hd, Lp, dtype=BF, device=DEV)
    out = torch.empty(B_, rows, D, dtype=BF, device=DEV)
    ws = torch.empty(hip_lib.attention_window_workspace_bytes(B_, H_, rows, hd), dtype=torch.uint8, device=DEV)

    def fill(flip):
        src_k, src_v = (v, k) if flip else (k, v)
        k_seg.copy_(_segments(src_k.to(DEV), P, Lc, 0, 0, 0.0))
        v_seg.copy_(_segments(src_v.to(DEV), P, Lc, 0, 0, 0.0))
        qr.copy_(q[:, row0: row0 + rows].to(DEV))

    def run():
        hip_lib.kv_join(k_seg, v_seg, kj, vtj, H_, hd, _L)
        hip_lib.attention_fwd_window(qr, kj, vtj, out, H_, hd, hd ** -0.5, n_prefix=_LT, windows=t, q_prescaled=True, workspace=ws)

    fill(False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                  # side-stream warm-up; also uploads the table outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    fill(True)                                                 # new operands: the replay must read them, join included
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    out.zero_()
    kj.zero_(), vtj.zero_()
    run()
    torch.cuda.synchronize()
    assert bool(replayed.float().abs().sum() > 0) and torch.isfinite(replayed.float()).all() and torch.equal(replayed, out)


# ----------------------------------------------------------------------------- 4. the model, ranks as threads
def _gpu_model(name, **over):
    from open_sora_amd import mmdit
    from oracle import configs

    cfg = dict(configs.GOLDEN[name][0], **over)
    model = mmdit.Flux(device_map="cuda:0", torch_dtype=BF, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=BF, device="cuda:0"), strict=True)
    return cfg, model


@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
def test_aligned_split_matches_the_single_device_windowed_forward(hip_lib, mode):
    """L_txt 256 + 6 frames x 128 tokens over P = 2: Lc = 512, a rank's blocks are the single-device blocks, W = 1"""
    cfg, model = _gpu_model("hd72_eager_split")
    inp = torch_inputs(cfg, 2, 6, 8, 16, 256, dtype=BF, device="cuda:0")
    model.set_attention_window(1, 128)
    with torch.inference_mode():
        single = model(**inp).float().cpu()
        model.set_attention_window(None)
        off = model(**inp).float().cpu()
    torch.cuda.synchronize()
    model.set_attention_window(1, 128)
    n_blocks = cfg["depth"] + cfg["depth_single_blocks"]
    with _Counting(hip_lib, ["kv_join", "attention_fwd_window", "attention_fwd", "attention_fwd_ragged"]) as cnt:
        res = _ranks_forward(model, inp, 2, mode, True)
    names = [c[0] for c in cnt.calls]
    assert names.count("kv_join") == 2 * 2 * n_blocks and names.count("attention_fwd") == 0 and names.count("attention_fwd_ragged") == 0
    assert names.count("attention_fwd_window") == 2 * 2 * n_blocks * (2 if mode == "ulysses" else 1)
    for outs, geom in res:
        assert geom == (512, 512) and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], res[0][0][0])
    e, sep = rel_l2(res[0][0][0], single), rel_l2(off, single)
    print(f"aligned P = 2 {mode}: relL2 sharded vs single-device windowed {e:.3e}; window on vs off on one device {sep:.3e}")
    assert torch.isfinite(res[0][0][0]).all() and e <= 2.0 ** -7, e


SPLITS = [(2, "allgather", "hd72_eager_split", {}), (2, "ulysses", "hd72_eager_split", {}), (3, "allgather", "hd72_eager_split", {}),
          (2, "allgather", "hd128_liger_split", {}), (3, "ulysses", "hd128_liger_split", dict(hidden_size=384, num_heads=3))]


@pytest.mark.parametrize("P,mode,name,over", SPLITS, ids=[f"P{p}-{m}-{n.split('_')[0]}" for p, m, n, _ in SPLITS])
def test_full_tables_match_the_sharded_forward_without_a_window(hip_lib, P, mode, name, over):
    """L = 64 + 6 x 96 = 640: P = 2 (Lc = 320, blocks that are not the single-device blocks) and P = 3 (ragged: 214, 214, 212; head
    exchange needs a head count 3 divides: the head_dim-128 model with 3 heads).  W = the frame count: every table is full"""
    cfg, model = _gpu_model(name, **over)
    inp = torch_inputs(cfg, 2, _T, 8, 12, _LT, dtype=BF, device="cuda:0")
    Lc = -(-_L // P)
    plain = _ranks_forward(model, inp, P, mode, True, n_fwd=1)
    model.set_attention_window(_T, _N)
    with _Counting(hip_lib, ["kv_join", "attention_fwd_window", "attention_fwd", "attention_fwd_ragged"]) as cnt:
        wide = _ranks_forward(model, inp, P, mode, True)
    names = [c[0] for c in cnt.calls]
    assert set(names) == {"kv_join", "attention_fwd_window"}, set(names)           # the ragged two-launch entry is not used on this path
    for outs, geom in wide:
        assert geom == (Lc, _L - (P - 1) * Lc) and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], wide[0][0][0])
    e = rel_l2(wide[0][0][0], plain[0][0][0])
    print(f"P = {P} {mode} {name}: relL2 sharded full windows vs sharded without a window {e:.3e}")
    assert torch.isfinite(wide[0][0][0]).all() and e <= 2.0 ** -7, e


def test_window_off_keeps_the_sharded_launches(hip_lib):
    """with the window off -- never set, and set then cleared -- a divisible split is one osk_attention_fwd_bounded_bf16 launch per
    block and rank over P segments, as before: no join, no window call"""
    P, (B, T, h, w, L_txt) = 2, (2, 4, 8, 8, 64)
    cfg, model = _gpu_model("hd72_eager_split")
    L = L_txt + T * h * w
    inp = torch_inputs(cfg, B, T, h, w, L_txt, dtype=BF, device="cuda:0")
    n_blocks = cfg["depth"] + cfg["depth_single_blocks"]
    outs = []
    for touch in (False, True):
        if touch:
            model.set_attention_window(1, h * w).set_attention_window(None)
        with _Counting(hip_lib, ["kv_join", "attention_fwd_window", "attention_fwd", "attention_fwd_ragged"]) as cnt:
            res = _ranks_forward(model, inp, P, "allgather", True, n_fwd=1)
        assert len(cnt.calls) == P * n_blocks and all(c == ("attention_fwd", P, L // P, None) for c in cnt.calls), cnt.calls[:3]
        outs.append(res[0][0][0])
    assert torch.equal(outs[0], outs[1])
