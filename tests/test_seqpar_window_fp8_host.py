"""CPU: frame-window attention under sequence parallelism in fp8 mode, host side.  The CPU statements of osk_kv_quant_rows_fp8 and
osk_kv_join_fp8 (tests/cpu_ops_sp_window_fp8.py) against "de-segment, then the k_pack_fp8 / v_transpose_fp8 statements", the entries'
declarations and argument checks, and -- P ranks as threads over tests/local_transport.py -- the sharded windowed fp8 forward in
both exchange modes: its calls per rank (one reducing collective in all-gather mode and none in head-exchange mode, the
quantisations, one join per block, the window calls with the rank's rows and mode), the gathered bytes, its result against the
sharded fp8 forward without a window and the single-device fp8 windowed forward, and what stays refused.  The kernels:
tests/test_gpu_seqpar_window_fp8.py."""
import copy
import os
import threading
import types

import pytest
import torch

from oracle import configs
from tests import cpu_ops_sp_window_fp8 as SF
from tests.local_transport import LocalTransport, LocalWorld, run_ranks
from tests.test_seqpar_qk8_host import SP_VS_SINGLE
from tests.util import rel_l2, torch_inputs, torch_params

BF = torch.bfloat16
U8 = torch.uint8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = SF.R


class CountingTransport(LocalTransport):
    """LocalTransport that counts its collectives and the bytes of every all-gather"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.n = {"all_reduce_max": 0, "all_gather": 0, "all_to_all": 0}
        self.gathered = []         # (dtype, bytes of the gathered buffer) per all-gather
        self.reduced = []          # shapes of the max-reduced buffers

    def all_reduce_max(self, t):
        self.n["all_reduce_max"] += 1
        self.reduced.append(tuple(t.shape))
        return super().all_reduce_max(t)

    def all_gather(self, out, inp):
        self.n["all_gather"] += 1
        self.gathered.append((out.dtype, out.numel() * out.element_size()))
        return super().all_gather(out, inp)

    def all_to_all(self, out, inp):
        self.n["all_to_all"] += 1
        return super().all_to_all(out, inp)


@pytest.fixture()
def sf_ops(hip_lib, monkeypatch):
    from open_sora_amd import mmdit

    monkeypatch.delenv("OSK_ATTN_WINDOW_FRAMES", raising=False)
    monkeypatch.delenv("OSK_ATTN_WINDOW_ANCHORS", raising=False)
    monkeypatch.delenv("OSK_SP_KV_CHUNKS", raising=False)
    mmdit.set_ops_for_testing(SF)
    SF.CALLS.clear()
    yield mmdit
    mmdit.set_ops_for_testing(hip_lib)


# ----------------------------------------------------------------------------- the two statements
def _segments(x, n_seg, seg_len, fill):
    """x [B, L, D] cut into segments inside a larger strided buffer; pad rows / columns and the rows behind the last key hold `fill`"""
    B, L, D = x.shape
    wide = torch.full((n_seg, B, seg_len + 3, D + 32), fill, dtype=x.dtype)
    seg = wide[:, :, :seg_len, 16: 16 + D]
    for s in range(n_seg):
        rows = x[:, s * seg_len: min((s + 1) * seg_len, L)]
        seg[s, :, :rows.shape[1]] = rows
    return seg


@pytest.mark.parametrize("hd,k8", [(72, False), (128, False), (128, True)])
@pytest.mark.parametrize("n_seg,seg_len,L", [(3, 100, 237), (2, 64, 128), (4, 33, 130), (1, 70, 70)])
def test_join_statement_is_desegment_then_pack_and_transpose(hd, k8, n_seg, seg_len, L):
    B, H = 2, 2
    D, Lp = H * hd, (L + 63) // 64 * 64
    g = torch.Generator().manual_seed(hd + L)
    k, v = torch.randn(B, L, D, generator=g).to(BF), (3.0 * torch.randn(B, L, D, generator=g)).to(BF)
    s2 = SF.kv_scale_fp8(k, v, H, hd)
    k_seg, v_seg = _segments(k, n_seg, seg_len, float("nan")), _segments(v, n_seg, seg_len, float("nan"))
    v8 = _segments(torch.zeros(B, L, D, dtype=U8), n_seg, seg_len, 0x7F)
    k8_seg = _segments(torch.zeros(B, L, D, dtype=U8), n_seg, seg_len, 0x7F)
    for s in range(n_seg):
        rows = min((s + 1) * seg_len, L) - s * seg_len
        SF.kv_quant_rows_fp8(v_seg[s][:, :rows], s2[1], v8[s][:, :rows], H, hd)
        if k8:
            SF.kv_quant_rows_fp8(k_seg[s][:, :rows], s2[0], k8_seg[s][:, :rows], H, hd)
    vt8 = torch.full((B, H, SF.vt8_rows(hd), Lp), 7, dtype=U8)
    k_out = torch.full(SF.k8_shape(B, H, L), 7, dtype=U8) if k8 else torch.full((B, L, D), 7.0, dtype=BF)
    SF.kv_join_fp8(k8_seg if k8 else k_seg, v8, k_out, vt8, H, hd, L)
    want_vt8 = SF.v_transpose_fp8(v, s2[1], torch.full((B, H, SF.vt8_rows(hd), Lp), 3, dtype=U8), H, hd)
    assert torch.equal(vt8, want_vt8)
    if k8:
        assert torch.equal(k_out, SF.k_pack_fp8(k, s2[0], torch.full(SF.k8_shape(B, H, L), 3, dtype=U8), H, hd))
        # the quantisation alone: the rows of the pack's output
        assert torch.equal(torch.cat([k8_seg[s] for s in range(n_seg)], 1)[:, :L].reshape(B, L, H, hd).permute(0, 2, 1, 3), k_out[:, :, :L])
    else:
        assert torch.equal(k_out.view(torch.int16), k.view(torch.int16))
    for bad_L in (n_seg * seg_len + 1, (n_seg - 1) * seg_len):
        if bad_L >= 1:
            with pytest.raises((RuntimeError, IndexError)):
                SF.kv_join_fp8(k8_seg if k8 else k_seg, v8, k_out, torch.empty(B, H, SF.vt8_rows(hd), (bad_L + 63) // 64 * 64, dtype=U8), H, hd, bad_L)


def test_entry_points_are_declared_bound_and_check_their_arguments(hip_lib):
    """status < 0 from the argument checks of the C entries, before any HIP call (no GPU here)"""
    with open(os.path.join(ROOT, "include", "osk.h")) as f:
        header = f.read()
    assert "int osk_kv_quant_rows_fp8(const void* x," in header and "int osk_kv_join_fp8(const void* k_seg," in header
    assert "#define OSK_ABI_VERSION 2" in header and hip_lib.lib.osk_abi_version() == 2
    assert len(hip_lib.SIGNATURES["osk_kv_quant_rows_fp8"]) == 12 and len(hip_lib.SIGNATURES["osk_kv_join_fp8"]) == 20
    f = hip_lib.lib.osk_kv_quant_rows_fp8
    ok = dict(x=0x1000, bs=25600, rs=256, s=0x3000, o=0x5000, obs=25600, ors=256, B=1, L=100, H=2, hd=128)
    call = lambda **kw: f(*[{**ok, **kw}[n] for n in ("x", "bs", "rs", "s", "o", "obs", "ors", "B", "L", "H", "hd")], None)
    for bad in (dict(x=None), dict(s=None), dict(o=None), dict(x=0x1008), dict(s=0x3002), dict(o=0x5008), dict(o=0x5004, hd=72, rs=144, ors=144),
                dict(rs=260), dict(bs=25604), dict(ors=264), dict(obs=25608), dict(ors=148, hd=72, rs=144), dict(B=0), dict(L=0), dict(H=0)):
        assert call(**bad) == -1, bad
    for hd in (64, 96, 256):
        assert call(hd=hd) == hip_lib.OSK_EUNSUPPORTED, hd
    j = hip_lib.lib.osk_kv_join_fp8
    ok = dict(k=0x1000, kss=25600, kbs=25600, krs=256, kind=1, v=0x9000, vss=25600, vbs=25600, vrs=256, ko=0x20000, kobs=0, kors=0,
              vt=0x40000, B=1, H=2, hd=128, n=3, sl=100, L=237)
    order = ("k", "kss", "kbs", "krs", "kind", "v", "vss", "vbs", "vrs", "ko", "kobs", "kors", "vt", "B", "H", "hd", "n", "sl", "L")
    call = lambda **kw: j(*[{**ok, **kw}[n] for n in order], None)
    for bad in (dict(L=0), dict(L=200), dict(L=301), dict(n=0), dict(n=2), dict(n=4), dict(sl=0), dict(sl=78), dict(sl=119), dict(B=0), dict(H=0),
                dict(k=None), dict(v=None), dict(ko=None), dict(vt=None), dict(kind=2), dict(kind=-1),
                dict(k=0x1008), dict(v=0x9008), dict(ko=0x20008), dict(vt=0x40008), dict(kss=25608), dict(krs=264), dict(vss=25608), dict(vbs=25608),
                dict(vrs=264), dict(kind=0, krs=260), dict(kind=0, kobs=4), dict(kind=0, kors=260), dict(hd=72, kind=0, v=0x9004)):
        assert call(**bad) == -1, bad
    for kw in (dict(hd=64, kind=0), dict(hd=96), dict(hd=72, kind=1)):
        assert call(**kw) == hip_lib.OSK_EUNSUPPORTED, kw
    # the binding's own checks raise before anything is launched (CPU tensors: a launch would fault, not raise)
    z = torch.zeros(2, 1, 64, 256, dtype=U8)
    with pytest.raises(AssertionError):
        hip_lib.kv_join_fp8(z, z, torch.zeros(1, 2, 128, 128, dtype=U8), torch.zeros(1, 2, 144, 192, dtype=U8), 2, 128, 128)
    with pytest.raises(AssertionError):
        hip_lib.kv_quant_rows_fp8(torch.zeros(1, 64, 256, dtype=BF), torch.ones(1, 2), torch.zeros(1, 64, 256, dtype=BF), 2, 128)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("kind,hd", SF.KIND_HD)
def test_emulation_passes_the_f64_check_of_the_gpu_rank_cases(hip_lib, kind, hd, P):
    """the operands, tables and tolerance tests/test_gpu_seqpar_window_fp8.py holds the kernels to: the torch emulation of the two
    launches and the merge stays inside, so the check is one a correct kernel can pass"""
    q, k, v, Lc, ranks = SF.rank_case(kind, hd, P)
    assert (Lc, ranks[-1][1]) == ((284, 284) if P == 2 else (190, 188))
    assert any(int(t[:, 1].min()) < (SF.R_N * SF.R_T + 63) // 64 for _, _, t, _ in ranks)
    for rank, (row0, rows, t, ref) in enumerate(ranks):
        r = R.ratios(*SF.emulate(q[:, row0: row0 + rows].contiguous(), k, v, SF.RH, hd, SF.R_LT, t, kind, "max"), ref)
        print(f"emulation {kind} hd {hd} P {P} rank {rank} table {t.tolist()}: err/tol {r[0]:.3f}  dlse/tol {r[1]:.3f}")
        assert r[0] <= 1.0 and r[1] <= 1.0, r


# ----------------------------------------------------------------------------- the model
_T, _h, _w, _LT = 6, 8, 12, 64                              # 64 text + 6 frames x 96 image tokens = 640 rows
_N = _h * _w
MODELS = {"pv8-hd72": ("hd72_eager_split", 72, False), "pv8-hd128": ("hd128_eager_fused", 128, False), "qk8-hd128": ("hd128_eager_fused", 128, True)}


def _heads(hd, divisor=1):
    """the smallest head count the model takes (hidden_size % 64 == 0) that `divisor` divides"""
    return {(72, 1): 8, (72, 2): 8, (128, 1): 2, (128, 2): 2, (128, 3): 3}[hd, divisor]


def _model(mmdit, which, heads=None):
    name, hd, qk8 = MODELS[which]
    heads = heads or _heads(hd)
    cfg = dict(configs.GOLDEN[name][0], depth=1, depth_single_blocks=1, hidden_size=hd * heads, num_heads=heads)
    model = mmdit.Flux(device_map="cpu", torch_dtype=BF, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=BF), strict=True)
    return cfg, model.enable_fp8(True, qk8=qk8), ("qk8" if qk8 else "pv8")


def _run_sp(model, inp, P, mode, sp_cls=None, **enable_kw):
    """-> per rank (prediction, the rank's recorded calls, its transport's counts, its SeqPar)"""
    from open_sora_amd import seqpar

    def rank_fn(rank, world):
        m = copy.copy(model)
        m.forward = m.forward_ckpt
        object.__setattr__(m, "_osk_ws_cache", {})
        tp = CountingTransport(world, rank, "cpu")
        sp = seqpar.enable(m, mode=mode, transport=tp, **enable_kw)
        with torch.inference_mode():
            out = m(**inp).float().clone()
        return out, threading.get_ident(), dict(tp.n, gathered=tp.gathered, reduced=tp.reduced), sp

    SF.CALLS.clear()
    res = run_ranks(P, rank_fn, "cpu")
    return [(out, list(SF.CALLS.get(ident, [])), n, sp) for out, ident, n, sp in res]


def _names(calls):
    return [c[0] for c in calls]


def _block_sequence(fmode, heads_mode, P):
    """the recorded entries of one block on one rank with the window on"""
    scale = ["kv_scale_fp8", "kv_quant_rows_fp8"] if fmode == "qk8" else ["v_scale_fp8"]
    return scale + ["kv_quant_rows_fp8", "kv_join_fp8"] + ["attention_fwd_window_fp8"] * (P if heads_mode else 1)


# (head_dim 72 over P = 3 in head-exchange mode needs 24 heads -- hidden_size % 64 == 0 -- and 20 s on the CPU: the ragged head exchange
#  runs in pv8 and qk8 at head_dim 128, head_dim 72 in every other combination)
CASES = [(which, P, mode) for which in MODELS for P in (2, 3) for mode in ("allgather", "ulysses") if (which, P, mode) != ("pv8-hd72", 3, "ulysses")]


@pytest.mark.parametrize("which,P,mode", CASES, ids=[f"{w}-P{p}-{m}" for w, p, m in CASES])
def test_full_windows_give_the_unwindowed_sharded_fp8_forward(sf_ops, which, P, mode):
    """L = 64 + 6 x 96 = 640 over P = 2 (Lc = 320) and P = 3 (ragged: 214, 214, 212).  W = the frame count: every table is full, so the
    sharded windowed fp8 forward sees every key with the scales and the e4m3 bytes of the sharded fp8 forward without a window; what
    differs is the two-launch merge and its second rounding -- held to the bound of a sharded fp8 forward (SP_VS_SINGLE).  W = 0
    must move the result."""
    hd = MODELS[which][1]
    heads = _heads(hd, P if mode == "ulysses" else 1)
    cfg, model, fmode = _model(sf_ops, which, heads)
    inp = torch_inputs(cfg, 2, _T, _h, _w, _LT, dtype=BF)
    L, Lc = 640, -(-640 // P)
    Ltail = L - (P - 1) * Lc
    heads_mode = mode == "ulysses"
    Hl = heads // P if heads_mode else heads
    plain = _run_sp(model, inp, P, mode)
    assert not any(n in ("kv_join_fp8", "kv_quant_rows_fp8", "attention_fwd_window_fp8") for _, calls, _, _ in plain for n in _names(calls))
    model.enable_fp8(False).set_attention_window(_T, _N)
    bf16_bytes = [n["gathered"] for _, _, n, _ in _run_sp(model, inp, P, mode)]
    model.enable_fp8(True, qk8=fmode == "qk8")               # either order: the window is on already
    wide = _run_sp(model, inp, P, mode)
    tiles = (L - _LT + 63) // 64
    rows = [Ltail if r == P - 1 else Lc for r in range(P)]
    for rank, (out, calls, n, sp) in enumerate(wide):
        assert sp.geom == (Lc, Ltail) and torch.equal(out, wide[0][0])
        assert _names(calls) == _block_sequence(fmode, heads_mode, P) * 2, _names(calls)       # a double and a single block
        assert "attention_fwd_ragged" not in _names(calls)
        assert [c for c in calls if c[0] == "kv_join_fp8"] == [("kv_join_fp8", P, Lc, L, Hl, "e4m3" if fmode == "qk8" else "bf16")] * 2
        wins = [c for c in calls if c[0] == "attention_fwd_window_fp8"]
        assert [c[2] for c in wins] == ([rows[rank]] * 2 if not heads_mode else rows * 2), wins
        assert all(c[1] == fmode and c[3:5] == (L, _LT) and all(r_ == (0, tiles) for r_ in c[5]) and len(c[5]) == (c[2] + 255) // 256 for c in wins)
        quants = [c for c in calls if c[0] == "kv_quant_rows_fp8"]
        assert all(c[1:] == ((P * 2, Lc, Hl, hd) if heads_mode else (2, rows[rank], Hl, hd)) for c in quants), quants
        # ONE reducing collective per block in all-gather mode, none in head-exchange mode
        assert n["all_reduce_max"] == (0 if heads_mode else 2), n
        if heads_mode:
            assert n["all_to_all"] == 8 and n["all_gather"] == 1, n
        else:
            assert n["reduced"] == [(2, 2, heads) if fmode == "qk8" else (2, heads)] * 2 and n["all_to_all"] == 0, n
            # every e4m3 operand travels at half the bytes of the bf16 window path: V always, K under qk8
            (kd, kb), (vd, vb), (_, kb16), (_, vb16) = n["gathered"][0], n["gathered"][1], bf16_bytes[rank][0], bf16_bytes[rank][1]
            assert len(n["gathered"]) == len(bf16_bytes[rank]) == 5 and n["gathered"][4] == bf16_bytes[rank][4]
            assert vd == U8 and 2 * vb == vb16 and ((kd, 2 * kb) == (U8, kb16) if fmode == "qk8" else (kd, kb) == (BF, kb16)), n["gathered"]
    if not heads_mode:      # every rank holds the scales of ALL heads: the same on every rank, call by call
        for a, b in zip(*[[c for c in calls if c[0] == "attention_fwd_window_fp8"] for _, calls, _, _ in wide[:2]]):
            assert torch.equal(a[7], b[7]) and (a[6] is None) == (fmode == "pv8") and (a[6] is None or torch.equal(a[6], b[6]))
    e = rel_l2(wide[0][0], plain[0][0])
    model.set_attention_window(0, _N)
    narrow = _run_sp(model, inp, P, mode)
    e0 = rel_l2(narrow[0][0], plain[0][0])
    print(f"{which} P = {P} {mode}: relL2 full windows vs no window {e:.3e}; W = 0 vs no window {e0:.3e}")
    assert e <= SP_VS_SINGLE and e0 > 2 * e, (e, e0)


ALIGNED = [(which, mode) for which in MODELS for mode in ("allgather", "ulysses")]


@pytest.mark.parametrize("which,mode", ALIGNED, ids=[f"{w}-{m}" for w, m in ALIGNED])
def test_aligned_split_is_the_single_device_windowed_fp8_forward(sf_ops, which, mode):
    """L_txt 256 + 6 frames x 128 tokens over P = 2: Lc = 512, a rank's 256-row blocks ARE the single-device blocks, W = 1.  The scales
    and the e4m3 bytes are the single device's by construction; the bound is the one a sharded fp8 forward is held to against the
    single process (SP_VS_SINGLE: the row chunking of the fp8 Linears' dynamic activation scales)."""
    from open_sora_amd.mmdit import attention_window_table

    cfg, model, fmode = _model(sf_ops, which)
    inp = torch_inputs(cfg, 1, 6, 8, 16, 256, dtype=BF)
    model.set_attention_window(1, 128)
    with torch.inference_mode():
        single = model(**inp).float().clone()
    res = _run_sp(model, inp, 2, mode)
    full = tuple(map(tuple, attention_window_table(256, 768, 128, 1).tolist()))
    for rank, (out, calls, n, sp) in enumerate(res):
        assert sp.geom == (512, 512) and torch.equal(out, res[0][0])
        wins = [c for c in calls if c[0] == "attention_fwd_window_fp8"]
        if mode == "allgather":
            assert [c[5] for c in wins] == [full[2 * rank: 2 * rank + 2]] * 2, wins
        else:
            assert [c[5] for c in wins] == [full[0:2], full[2:4]] * 2, wins
        assert all(c[1:5] == (fmode, 512, 1024, 256) for c in wins)
    e = rel_l2(res[0][0], single)
    print(f"aligned P = 2 {which} {mode}: relL2 sharded vs single-device windowed fp8 {e:.3e}")
    assert e <= SP_VS_SINGLE, e


@pytest.mark.parametrize("which,mode", [("pv8-hd72", "allgather"), ("qk8-hd128", "ulysses")])
def test_anchors_take_the_anchored_entry_in_the_fp8_mode(sf_ops, which, mode):
    from open_sora_amd.mmdit import attention_window_bounds

    cfg, model, fmode = _model(sf_ops, which)
    inp = torch_inputs(cfg, 1, _T, _h, _w, _LT, dtype=BF)
    model.set_attention_window(1, _N, anchors=(1, 1))
    res = _run_sp(model, inp, 2, mode)
    bounds = attention_window_bounds(_LT, _T * _N, _N, 1, 1)
    for out, calls, n, sp in res:
        assert torch.equal(out, res[0][0]) and torch.isfinite(out).all()
        names = _names(calls)
        assert "attention_fwd_window_fp8" not in names and names.count("kv_join_fp8") == 2
        wins = [c for c in calls if c[0] == "attention_fwd_window_anchor"]
        assert len(wins) == (4 if mode == "ulysses" else 2) and all(c[1] == fmode and c[3] == 640 and c[4:6] == tuple(bounds) for c in wins), wins


def test_window_off_keeps_the_calls_of_the_unwindowed_fp8_forward(sf_ops):
    for which, mode in (("qk8-hd128", "allgather"), ("pv8-hd72", "ulysses")):
        cfg, model, fmode = _model(sf_ops, which)
        inp = torch_inputs(cfg, 1, _T, _h, _w, _LT, dtype=BF)
        before = _run_sp(model, inp, 2, mode)
        model.set_attention_window(1, _N).set_attention_window(None)
        after = _run_sp(model, inp, 2, mode)
        for (o0, c0, n0, _), (o1, c1, n1, _) in zip(before, after):
            assert c0 == c1 and n0 == n1 and torch.equal(o0, o1)
            assert not {"kv_join_fp8", "kv_quant_rows_fp8", "attention_fwd_window_fp8"} & set(_names(c0))
            assert ("attention_fwd_qk8" if fmode == "qk8" else "attention_fwd_pv8") in _names(c0)


def test_what_stays_refused(sf_ops):
    from open_sora_amd import seqpar

    cfg, model, fmode = _model(sf_ops, "pv8-hd72")
    tp = lambda: LocalTransport(LocalWorld(2), 0, "cpu")
    inp = torch_inputs(cfg, 1, _T, _h, _w, _LT, dtype=BF)
    # accepted, both orders
    seqpar.enable(model, mode="allgather", transport=tp())
    assert model.set_attention_window(1, _N)._attn_window == (1, _N)
    model.enable_fp8(False)
    assert model.enable_fp8(True) is model
    # kv_chunks > 1
    seqpar.enable(model, mode="allgather", transport=tp(), kv_chunks=2)
    with torch.inference_mode(), pytest.raises(ValueError, match="kv_chunks"):
        model(**inp)
    # the step cache
    seqpar.enable(model, mode="allgather", transport=tp())
    with pytest.raises(ValueError, match="step_cache"):
        model.step_cache_begin(1, 3, _T * _N, "cpu")
    # a kernel table without the new entries: every order refuses with "fp8", before any launch
    for missing in ("kv_join_fp8", "kv_quant_rows_fp8"):
        sf_ops.set_ops_for_testing(types.SimpleNamespace(**{k: v for k, v in vars(SF).items() if k != missing}))
        with torch.inference_mode(), pytest.raises(ValueError, match="fp8"):
            model(**inp)
        model.enable_fp8(False)
        with pytest.raises(ValueError, match="fp8"):
            model.enable_fp8(True)
        model.set_attention_window(None)
        model.enable_fp8(True)
        with pytest.raises(ValueError, match="fp8"):
            model.set_attention_window(1, _N)
        with pytest.raises(ValueError, match="fp8"):
            seqpar.SeqPar(mode="allgather", transport=tp())._window_kv_start(torch.zeros(1, 320, 576, dtype=BF), torch.zeros(1, 320, 576, dtype=BF),
                                                                            8, 72, True, False, (_LT, _T * _N, 1, _N))
        sf_ops.set_ops_for_testing(SF)
        model.set_attention_window(1, _N)
    # an sp object from before the fp8 window path
    class OldSeqPar(seqpar.SeqPar):
        kv_window_fp8 = False

    model._sp = OldSeqPar(mode="allgather", transport=tp())
    with torch.inference_mode(), pytest.raises(ValueError, match="fp8"):
        model(**inp)
    model.set_attention_window(None)
    with pytest.raises(ValueError, match="fp8"):
        model.set_attention_window(1, _N)
    assert not SF.CALLS
