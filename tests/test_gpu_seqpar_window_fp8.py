"""GPU: frame-window attention under sequence parallelism in fp8 mode.
1. osk_kv_quant_rows_fp8 -> osk_kv_join_fp8 bit for bit: vt8 == osk_v_transpose_fp8 of the de-segmented V, k8 == osk_k_pack_fp8 of the
   de-segmented K (the bf16 K kind: K itself), with the same scales, as bytes; head_dim 72 (K bf16) and 128 (both K kinds),
   tile-misaligned segments and a short last segment, L % 64 zero and non-zero, inputs inside larger strided buffers whose pad rows /
   columns hold bf16 NaN or e4m3 0x7F, outputs inside guard bands; the quantisation alone == the rows of osk_k_pack_fp8's output.
2. every refused argument of both entries returns its code and leaves the outputs at their fill; the valid call returns 0.
3. one rank's quantise -> join -> window path, L_txt 64 + 7 frames x 72 tokens = 568 keys, W = 1, P = 2 (284 / 284) and P = 3 (190 / 190 /
   188), pv8 at head_dim 72 / 128 and qk8 at 128: output and LSE per element against the f64 reference on the e4m3 operands over each
   block's stated key set with the derived tolerance of tests/cpu_ops_window_fp8.py (the CPU suite shows the emulation passing the
   same check), and, with V the indicator of a key's tile, exactly zero mass outside a block's key set.
4. join + window call captured in a torch.cuda.graph and replayed == the eager pair after the operands changed.
5. the model with P ranks as threads (tests/local_transport.py), fp8 on, both exchange modes: an aligned split against the
   single-device fp8 windowed forward, a ragged P = 3 split with full tables against the sharded fp8 forward without a window, one
   anchored case -- within the 2e-2 tests/test_gpu_seqpar_qk8.py holds a sharded fp8 forward to -- with the launch counts.
Each check prints its figures before it asserts."""
import pytest
import torch

from tests import cpu_ops_sp_window_fp8 as SF
from tests.test_gpu_seqpar_ragged import GUARD, _Counting, _guarded, _guards_intact, _ranks_forward
from tests.test_gpu_seqpar_window import _gpu_model, _segments
from tests.util import rel_l2, torch_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
U8 = torch.uint8
R = SF.R
EINVAL = -1
SP_FP8 = 2e-2          # tests/test_gpu_seqpar_qk8.py: a sharded fp8 forward against the single device
KINDS = [(72, "pv8"), (128, "pv8"), (128, "qk8")]
H_, B_ = SF.RH, SF.RB


def _byte_segments(B, D, n_seg, seg_len):
    """uint8 [n_seg, B, seg_len, D] view inside a larger buffer; everything, pad rows and columns included, holds e4m3 NaN (0x7F)"""
    wide = torch.full((n_seg, B, seg_len + 3, D + 32), 0x7F, dtype=U8, device=DEV)
    return wide, wide[:, :, :seg_len, 16: 16 + D]


def _quantised(hip_lib, x_seg, scales, L, H, hd):
    """the bf16 segments of a tensor of L keys -> e4m3 segments (osk_kv_quant_rows_fp8 per segment, its valid rows only)"""
    n_seg, B, seg_len, D = x_seg.shape
    wide, seg8 = _byte_segments(B, D, n_seg, seg_len)
    for s in range(n_seg):
        rows = min((s + 1) * seg_len, L) - s * seg_len
        hip_lib.kv_quant_rows_fp8(x_seg[s][:, :rows], scales, seg8[s][:, :rows], H, hd)
    return wide, seg8


def _joined(hip_lib, k, v, hd, kind, n_seg, seg_len):
    """device (k operand, k_scale | None, vt8, v_scale) of k, v [B, L, D] through segments -> quantise -> join"""
    B, L, D = k.shape
    H = D // hd
    kd, vd = k.to(DEV), v.to(DEV)
    s2 = hip_lib.kv_scale_fp8(kd, vd, H, hd)
    k_seg, v_seg = _segments(kd, n_seg, seg_len), _segments(vd, n_seg, seg_len)
    _, v8 = _quantised(hip_lib, v_seg, s2[1], L, H, hd)
    vtj = torch.empty(B, H, hip_lib.vt8_rows(hd), (L + 63) // 64 * 64, dtype=U8, device=DEV)
    if kind == "qk8":
        _, k_seg = _quantised(hip_lib, k_seg, s2[0], L, H, hd)
        kj = torch.empty(hip_lib.k8_shape(B, H, L, hd), dtype=U8, device=DEV)
    else:
        kj = torch.empty(B, L, D, dtype=BF, device=DEV)
    hip_lib.kv_join_fp8(k_seg, v8, kj, vtj, H, hd, L)
    return kj, (s2[0] if kind == "qk8" else None), vtj, s2[1]


# ----------------------------------------------------------------------------- 1. the chain, bit for bit
@pytest.mark.parametrize("n_seg,seg_len,L", [(3, 100, 237), (2, 64, 128), (4, 33, 130)])
@pytest.mark.parametrize("hd,kind", KINDS)
def test_quantise_then_join_is_bit_exact(hip_lib, hd, kind, n_seg, seg_len, L):
    B, H = 2, 2
    D, Lp, RP = H * hd, (L + 63) // 64 * 64, hip_lib.vt8_rows(hd)
    g = torch.Generator(device=DEV).manual_seed(hd + L)
    k = torch.randn(B, L, D, device=DEV, generator=g).to(BF)
    v = (3.0 * torch.randn(B, L, D, device=DEV, generator=g)).to(BF)
    s2 = hip_lib.kv_scale_fp8(k, v, H, hd)
    k_seg, v_seg = _segments(k, n_seg, seg_len), _segments(v, n_seg, seg_len)        # pad rows / columns: bf16 NaN
    v_wide, v8 = _quantised(hip_lib, v_seg, s2[1], L, H, hd)
    vt_raw, vt8, vt_pad = _guarded((B, H, RP, Lp), U8)
    if kind == "qk8":
        k_wide, k_in = _quantised(hip_lib, k_seg, s2[0], L, H, hd)
        ko_raw, k_out, ko_pad = _guarded(hip_lib.k8_shape(B, H, L, hd), U8)
    else:
        k_in = k_seg
        ko_raw, ko_wide, ko_pad = _guarded((B, L, D + 8), BF)
        k_out = ko_wide[:, :, :D]                                  # a view with strides of its own
    hip_lib.kv_join_fp8(k_in, v8, k_out, vt8, H, hd, L)
    want_vt8 = hip_lib.v_transpose_fp8(v, s2[1], torch.full((B, H, RP, Lp), 3, dtype=U8, device=DEV), H, hd)
    torch.cuda.synchronize()
    assert _guards_intact(ko_raw, ko_pad) and _guards_intact(vt_raw, vt_pad)
    # the quantisation wrote its rows and nothing else: pad rows, pad columns and the rows behind key L - 1 keep their 0x7F
    mask = torch.ones_like(v_wide, dtype=torch.bool)
    for s in range(n_seg):
        mask[s, :, : min((s + 1) * seg_len, L) - s * seg_len, 16: 16 + D] = False
    assert bool((v_wide[mask] == 0x7F).all()), "osk_kv_quant_rows_fp8 wrote outside its rows"
    assert torch.equal(vt8, want_vt8)
    if kind == "qk8":
        want_k8 = hip_lib.k_pack_fp8(k, s2[0], torch.full(hip_lib.k8_shape(B, H, L, hd), 3, dtype=U8, device=DEV), H, hd)
        torch.cuda.synchronize()
        assert bool((k_wide[mask] == 0x7F).all())
        assert torch.equal(k_out, want_k8)
        # the quantisation alone: token-major rows == the rows of the pack's output
        flat = torch.full((B, L, D), 0x7F, dtype=U8, device=DEV)
        hip_lib.kv_quant_rows_fp8(k, s2[0], flat, H, hd)
        torch.cuda.synchronize()
        assert torch.equal(flat.view(B, L, H, hd).permute(0, 2, 1, 3), want_k8[:, :, :L])
    else:
        assert bool((ko_wide[:, :, D:].view(U8) == GUARD).all()), "the columns beside k_out were written"
        assert torch.equal(k_out.view(torch.int16), k.view(torch.int16))


# ----------------------------------------------------------------------------- 2. status codes
def test_status_codes(hip_lib):
    """every refused call returns its code and launches nothing: the outputs keep their fill"""
    B, H, hd, n_seg, seg_len, L = 1, 2, 128, 3, 100, 237
    D, Lp = H * hd, 256
    st = torch.cuda.current_stream().cuda_stream
    x = torch.ones(B, L, D, dtype=BF, device=DEV)
    sc = torch.ones(B, H, device=DEV)
    o8 = torch.full((B, L, D), 0x7F, dtype=U8, device=DEV)

    def quant(x_=x.data_ptr(), bs=x.stride(0), rs=x.stride(1), s=sc.data_ptr(), o=o8.data_ptr(), obs=o8.stride(0), ors=o8.stride(1), B_=B, L_=L, H_=H, hd_=hd):
        return hip_lib.lib.osk_kv_quant_rows_fp8(x_, bs, rs, s, o, obs, ors, B_, L_, H_, hd_, st)

    for kw in (dict(x_=None), dict(s=None), dict(o=None), dict(x_=x.data_ptr() + 8), dict(s=sc.data_ptr() + 2), dict(o=o8.data_ptr() + 8),
               dict(o=o8.data_ptr() + 4, hd_=72), dict(rs=D + 4), dict(bs=x.stride(0) + 4), dict(ors=D + 8), dict(obs=o8.stride(0) + 8),
               dict(ors=D + 4, hd_=72), dict(B_=0), dict(L_=0), dict(H_=0)):
        assert quant(**kw) == EINVAL, kw
    for hd_ in (64, 96, 256):
        assert quant(hd_=hd_) == hip_lib.OSK_EUNSUPPORTED, hd_
    torch.cuda.synchronize()
    assert bool((o8 == 0x7F).all())
    assert quant() == 0
    torch.cuda.synchronize()
    assert bool((o8 == 0x38).all())                                  # 1.0 / 1.0 -> e4m3 1.0

    seg8 = torch.zeros(n_seg, B, seg_len, D, dtype=U8, device=DEV)
    segb = torch.zeros(n_seg, B, seg_len, D, dtype=BF, device=DEV)
    k8o = torch.full((B, H, Lp, 128), 3, dtype=U8, device=DEV)
    kbo = torch.full((B, L, D), 3.0, dtype=BF, device=DEV)
    vto = torch.full((B, H, hip_lib.vt8_rows(hd), Lp), 3, dtype=U8, device=DEV)

    def join(k=seg8.data_ptr(), kss=seg8.stride(0), kbs=seg8.stride(1), krs=seg8.stride(2), kind=1, v=seg8.data_ptr(), vss=seg8.stride(0),
             vbs=seg8.stride(1), vrs=seg8.stride(2), ko=k8o.data_ptr(), kobs=0, kors=0, vt=vto.data_ptr(), B_=B, H_=H, hd_=hd, n=n_seg, sl=seg_len, L_=L):
        return hip_lib.lib.osk_kv_join_fp8(k, kss, kbs, krs, kind, v, vss, vbs, vrs, ko, kobs, kors, vt, B_, H_, hd_, n, sl, L_, st)

    bf = dict(k=segb.data_ptr(), kss=segb.stride(0), kbs=segb.stride(1), krs=segb.stride(2), kind=0, ko=kbo.data_ptr(), kobs=kbo.stride(0), kors=kbo.stride(1))
    bad = [dict(L_=0), dict(L_=200), dict(L_=301), dict(n=0), dict(n=2), dict(n=4), dict(sl=0), dict(sl=78), dict(sl=119), dict(B_=0), dict(H_=0),
           dict(k=None), dict(v=None), dict(ko=None), dict(vt=None), dict(kind=2), dict(kind=-1),
           dict(k=seg8.data_ptr() + 8), dict(v=seg8.data_ptr() + 8), dict(ko=k8o.data_ptr() + 8), dict(vt=vto.data_ptr() + 8),
           dict(kss=seg8.stride(0) + 8), dict(kbs=seg8.stride(1) + 8), dict(krs=D + 8), dict(vss=seg8.stride(0) + 8), dict(vbs=seg8.stride(1) + 8),
           dict(vrs=D + 8), dict(bf, krs=D + 4), dict(bf, kss=segb.stride(0) + 4), dict(bf, kobs=kbo.stride(0) + 4), dict(bf, kors=D + 4),
           dict(bf, k=segb.data_ptr() + 8), dict(bf, ko=kbo.data_ptr() + 8), dict(bf, hd_=72, v=seg8.data_ptr() + 4), dict(bf, hd_=72, vrs=D + 4)]
    for kw in bad:
        assert join(**kw) == EINVAL, kw
    for kw in (dict(bf, hd_=64), dict(hd_=96), dict(bf, hd_=256), dict(hd_=72)):
        assert join(**kw) == hip_lib.OSK_EUNSUPPORTED, kw
    torch.cuda.synchronize()
    assert bool((k8o == 3).all()) and bool((kbo == 3.0).all()) and bool((vto == 3).all())
    assert join() == 0 and join(**bf) == 0
    torch.cuda.synchronize()
    assert bool((k8o == 0).all()) and bool((kbo == 0).all())
    # the validity row: 0x38 at the positions of the L keys (the last tile in the kernel's key order), 0 at the others
    ones = vto[:, :, hd]
    assert bool((vto[:, :, :hd] == 0).all()) and bool((vto[:, :, hd + 1:] == 0).all()) and bool((ones[..., : L // 64 * 64] == 0x38).all())
    assert bool(((ones == 0x38) | (ones == 0)).all()) and int((ones == 0x38).sum()) == B * H * L


# ----------------------------------------------------------------------------- 3. one rank's quantise -> join -> window path
def _window_call(hip_lib, q, ops, hd, kind, table, lse=True):
    kj, sk, vtj, sv = ops
    out = torch.full_like(q, float("nan"))
    l = torch.full((q.shape[0], H_, q.shape[1]), float("nan"), device=DEV) if lse else None
    hip_lib.attention_fwd_window_fp8(q, kj, sk, vtj, sv, out, H_, hd, hd ** -0.5, n_prefix=SF.R_LT, windows=table, mode=kind, lse=l,
                                     q_prescaled=True, Lk=SF.R_L)
    torch.cuda.synchronize()
    return out.cpu(), None if l is None else l.cpu()


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("hd,kind", KINDS)
def test_rank_quantise_join_window_vs_f64(hip_lib, hd, kind, P):
    q, k, v, Lc, ranks = SF.rank_case(kind, hd, P)
    tiles = (SF.R_N * SF.R_T + 63) // 64
    assert (Lc, ranks[-1][1]) == ((284, 284) if P == 2 else (190, 188))
    assert any(int(t[:, 1].min()) < tiles for _, _, t, _ in ranks), "no block whose range is short of the full body"
    ops = _joined(hip_lib, k, v, hd, kind, P, Lc)
    qd = q.to(DEV)
    worst = 0.0
    for rank, (row0, rows, t, ref) in enumerate(ranks):
        out, lse = _window_call(hip_lib, qd[:, row0: row0 + rows], ops, hd, kind, t)
        finite = bool(torch.isfinite(out.float()).all() and torch.isfinite(lse).all())
        r = R.ratios(R.heads(out.float(), H_, hd), lse, ref)
        print(f"quantise -> join -> window {kind} hd {hd} P {P} rank {rank} rows [{row0}, {row0 + rows}) table {t.tolist()}: finite {finite}  "
              f"err/tol {r[0]:.3f}  dlse/tol {r[1]:.3f}")
        assert finite
        worst = max(worst, *r)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("hd,kind", KINDS)
def test_rank_path_puts_no_mass_outside_a_blocks_key_set(hip_lib, hd, kind):
    """tests/test_gpu_attention_window_fp8.py's tile indicator through the quantise -> join path: V[key, d] = 1 where key lies in body
    tile d (d < 8), V[key, 9] = 1 for a text key, 0 elsewhere -- every value and the scale 1 / 448 exact in e4m3, so out[row, d] is the
    mass the row put on tile d, exactly 0 for a tile outside its block's range; diffuse scores (below 1 log2 unit), so 'at least half
    of the f64 mass' inside cannot fail for any reason but the mask or the key order of the joined V^T"""
    P = 3
    _, _, _, Lc, ranks = SF.rank_case(kind, hd, P)
    L, LT = SF.R_L, SF.R_LT
    tiles = (L - LT + 63) // 64
    g = torch.Generator().manual_seed(31 * hd)
    k = torch.randn(B_, L, H_ * hd, generator=g).to(BF)
    q = torch.randn(B_, L, H_ * hd, generator=g)
    kn = k.float().reshape(B_, L, H_, hd).norm(dim=-1).max()
    q = (q * (0.9 / float(q.reshape(B_, L, H_, hd).norm(dim=-1).max() * kn))).to(BF)
    v = torch.zeros(B_, L, H_, hd)
    v[:, :LT, :, 9] = 1.0
    for j in range(tiles):
        v[:, LT + 64 * j: LT + 64 * (j + 1), :, j] = 1.0
    v = v.reshape(B_, L, H_ * hd).to(BF)
    ops = _joined(hip_lib, k, v, hd, kind, P, Lc)
    assert bool((ops[3] == 1.0 / 448.0).all())
    qm, km, _, _, _ = SF.mfma_operands(q, k, v, H_, hd, kind)
    s = qm.double() @ km.double().transpose(-1, -2)
    assert float(s.abs().max()) < 1.0
    qd = q.to(DEV)
    for rank, (row0, rows, t, _) in enumerate(ranks):
        out, _ = _window_call(hip_lib, qd[:, row0: row0 + rows], ops, hd, kind, t, lse=False)
        o = R.heads(out.float(), H_, hd).double()
        lo = 1.0
        for i, (first, n) in enumerate(t.tolist()):
            blk = slice(256 * i, min(256 * (i + 1), rows))
            keys = SF.block_keys(LT, L, first, n)
            p = torch.softmax(s[:, :, row0 + blk.start: row0 + blk.stop][..., keys] * R.LN2, -1)
            inside = [9] + list(range(first, first + n))
            stray = o[:, :, blk][..., [d for d in range(hd) if d not in inside]].abs().max().item()
            print(f"tile indicator {kind} hd {hd} rank {rank} block {i} ({first}, {n}): largest value outside the key set {stray:.3e}")
            assert stray == 0.0, (rank, i, stray)
            for d in inside:
                sel = keys < LT if d == 9 else (keys >= LT + 64 * d) & (keys < LT + 64 * (d + 1))
                lo = min(lo, (o[:, :, blk, d] / p[..., sel].sum(-1)).min().item())
        print(f"tile indicator {kind} hd {hd} rank {rank}: smallest (kernel mass / f64 mass) inside the key sets {lo:.3f}")
        assert lo >= 0.5, (rank, lo)


# ----------------------------------------------------------------------------- 4. capture
def test_join_and_window_call_replay_from_a_graph(hip_lib):
    hd, kind, P = 128, "qk8", 3
    q, k, v, Lc, ranks = SF.rank_case(kind, hd, P)
    row0, rows, t, _ = ranks[1]
    L, D = SF.R_L, H_ * hd
    k_seg, v_seg = torch.zeros(P, B_, Lc, D, dtype=U8, device=DEV), torch.zeros(P, B_, Lc, D, dtype=U8, device=DEV)
    s2 = torch.empty(2, B_, H_, device=DEV)
    qr = torch.empty(B_, rows, D, dtype=BF, device=DEV)
    kj = torch.empty(hip_lib.k8_shape(B_, H_, L, hd), dtype=U8, device=DEV)
    vtj = torch.empty(B_, H_, hip_lib.vt8_rows(hd), (L + 63) // 64 * 64, dtype=U8, device=DEV)
    out = torch.empty(B_, rows, D, dtype=BF, device=DEV)
    ws = torch.empty(hip_lib.attention_window_workspace_bytes(B_, H_, rows, hd), dtype=U8, device=DEV)

    def fill(flip):
        src_k, src_v = ((v, k) if flip else (k, v))
        kd, vd = src_k.to(DEV), src_v.to(DEV)
        hip_lib.kv_scale_fp8(kd, vd, H_, hd, out=s2)
        for x, seg in ((kd, k_seg), (vd, v_seg)):
            for s_ in range(P):
                n = min((s_ + 1) * Lc, L) - s_ * Lc
                hip_lib.kv_quant_rows_fp8(x[:, s_ * Lc: s_ * Lc + n], s2[0] if seg is k_seg else s2[1], seg[s_][:, :n], H_, hd)
        qr.copy_(q[:, row0: row0 + rows].to(DEV))

    def run():
        hip_lib.kv_join_fp8(k_seg, v_seg, kj, vtj, H_, hd, L)
        hip_lib.attention_fwd_window_fp8(qr, kj, s2[0], vtj, s2[1], out, H_, hd, hd ** -0.5, n_prefix=SF.R_LT, windows=t, mode=kind,
                                         q_prescaled=True, workspace=ws, Lk=L)

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


# ----------------------------------------------------------------------------- 5. the model, ranks as threads
NAMES = ["kv_join", "kv_join_fp8", "kv_quant_rows_fp8", "attention_fwd_window", "attention_fwd_window_fp8", "attention_fwd_window_anchor",
         "attention_fwd_pv8", "attention_fwd_qk8", "attention_fwd_ragged", "k_pack_fp8", "v_transpose_fp8"]
_T, _N, _LT = 6, 96, 64
_L = _LT + _T * _N


def _fp8_model(name, qk8, **over):
    cfg, model = _gpu_model(name, **over)
    return cfg, model.enable_fp8(True, qk8=qk8)


def _expected(n_blocks, P, mode, qk8, entry="attention_fwd_window_fp8"):
    """calls of P ranks x 2 forwards: per block a join, the quantisations (V; K too under qk8) and the window call(s)"""
    per_rank = 2 * n_blocks
    return {"kv_join_fp8": P * per_rank, "kv_quant_rows_fp8": P * per_rank * (2 if qk8 else 1), entry: P * per_rank * (P if mode == "ulysses" else 1)}


ALIGNED = [("hd72_eager_split", False, "allgather"), ("hd72_eager_split", False, "ulysses"), ("hd128_liger_split", True, "allgather"),
           ("hd128_liger_split", True, "ulysses")]


@pytest.mark.parametrize("name,qk8,mode", ALIGNED, ids=[f"{n.split('_')[0]}-{'qk8' if q else 'pv8'}-{m}" for n, q, m in ALIGNED])
def test_aligned_split_matches_the_single_device_windowed_fp8_forward(hip_lib, name, qk8, mode):
    """L_txt 256 + 6 frames x 128 tokens over P = 2: Lc = 512, a rank's blocks are the single-device blocks, W = 1"""
    cfg, model = _fp8_model(name, qk8)
    inp = torch_inputs(cfg, 2, 6, 8, 16, 256, dtype=BF, device="cuda:0")
    model.set_attention_window(1, 128)
    with torch.inference_mode():
        single = model(**inp).float().cpu()
    torch.cuda.synchronize()
    n_blocks = cfg["depth"] + cfg["depth_single_blocks"]
    with _Counting(hip_lib, NAMES) as cnt:
        res = _ranks_forward(model, inp, 2, mode, True)
    names = [c[0] for c in cnt.calls]
    assert {n: names.count(n) for n in set(names)} == _expected(n_blocks, 2, mode, qk8), {n: names.count(n) for n in set(names)}
    for outs, geom in res:
        assert geom == (512, 512) and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], res[0][0][0])
    e = rel_l2(res[0][0][0], single)
    print(f"aligned P = 2 {name} {'qk8' if qk8 else 'pv8'} {mode}: relL2 sharded vs single-device windowed fp8 {e:.3e}")
    assert torch.isfinite(res[0][0][0]).all() and e <= SP_FP8, e


RAGGED = [("hd72_eager_split", False, "allgather", {}), ("hd128_liger_split", True, "allgather", {}),
          ("hd128_liger_split", True, "ulysses", dict(hidden_size=384, num_heads=3)), ("hd128_liger_split", False, "ulysses", dict(hidden_size=384, num_heads=3))]


@pytest.mark.parametrize("name,qk8,mode,over", RAGGED, ids=[f"{n.split('_')[0]}-{'qk8' if q else 'pv8'}-{m}" for n, q, m, _ in RAGGED])
def test_ragged_full_tables_match_the_sharded_fp8_forward_without_a_window(hip_lib, name, qk8, mode, over):
    """L = 64 + 6 x 96 = 640 over P = 3 (214, 214, 212; head exchange needs a head count 3 divides: the head_dim-128 model with 3
    heads).  W = the frame count: every table is full"""
    P = 3
    cfg, model = _fp8_model(name, qk8, **over)
    inp = torch_inputs(cfg, 2, _T, 8, 12, _LT, dtype=BF, device="cuda:0")
    Lc = -(-_L // P)
    plain = _ranks_forward(model, inp, P, mode, True, n_fwd=1)
    model.set_attention_window(_T, _N)
    n_blocks = cfg["depth"] + cfg["depth_single_blocks"]
    with _Counting(hip_lib, NAMES) as cnt:
        wide = _ranks_forward(model, inp, P, mode, True)
    names = [c[0] for c in cnt.calls]
    assert {n: names.count(n) for n in set(names)} == _expected(n_blocks, P, mode, qk8), {n: names.count(n) for n in set(names)}   # no ragged two-launch entry
    for outs, geom in wide:
        assert geom == (Lc, _L - (P - 1) * Lc) and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], wide[0][0][0])
    e = rel_l2(wide[0][0][0], plain[0][0][0])
    print(f"P = 3 {mode} {name} {'qk8' if qk8 else 'pv8'}: relL2 sharded full windows vs sharded fp8 without a window {e:.3e}")
    assert torch.isfinite(wide[0][0][0]).all() and e <= SP_FP8, e


def test_anchored_split_matches_the_single_device_anchored_fp8_forward(hip_lib):
    """anchors (1, 1) on the aligned split (all-gather mode, qk8): the anchored entry in mode qk8 on the joined operands"""
    cfg, model = _fp8_model("hd128_liger_split", True)
    inp = torch_inputs(cfg, 2, 6, 8, 16, 256, dtype=BF, device="cuda:0")
    model.set_attention_window(1, 128, anchors=(1, 1))
    with torch.inference_mode():
        single = model(**inp).float().cpu()
    torch.cuda.synchronize()
    n_blocks = cfg["depth"] + cfg["depth_single_blocks"]
    with _Counting(hip_lib, NAMES) as cnt:
        res = _ranks_forward(model, inp, 2, "allgather", True)
    names = [c[0] for c in cnt.calls]
    assert {n: names.count(n) for n in set(names)} == _expected(n_blocks, 2, "allgather", True, "attention_fwd_window_anchor")
    for outs, geom in res:
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], res[0][0][0])
    e = rel_l2(res[0][0][0], single)
    print(f"anchored (1, 1) aligned P = 2 qk8 allgather: relL2 sharded vs single-device anchored fp8 {e:.3e}")
    assert torch.isfinite(res[0][0][0]).all() and e <= SP_FP8, e
