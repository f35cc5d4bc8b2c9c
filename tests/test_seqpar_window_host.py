"""CPU: frame-window attention under sequence parallelism, host side.  The rank-offset tables of mmdit.attention_window_table
(row0 / n_rows), the CPU statement of osk_kv_join_bf16 (tests/cpu_ops_sp_window.py) against "de-segment, then the V transpose of
tests/cpu_ops.py", the entry's declaration and binding, the refusals that remain, and -- P ranks as threads over
tests/local_transport.py on the CPU statements of the kernels -- the sharded windowed forward in both exchange modes: its calls
(one join per block, one window call per rank or per source rank, the table of the rows in hand) and its result against the
single-device windowed forward.  The kernels: tests/test_gpu_seqpar_window.py."""
import copy
import os
import threading
import types

import pytest
import torch

from oracle import configs
from tests import cpu_ops
from tests import cpu_ops_sp_window as SW
from tests.local_transport import LocalTransport, run_ranks
from tests.util import rel_l2, torch_inputs, torch_params

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def sw_ops(hip_lib, monkeypatch):
    from open_sora_amd import mmdit

    monkeypatch.delenv("OSK_ATTN_WINDOW_FRAMES", raising=False)
    monkeypatch.delenv("OSK_SP_KV_CHUNKS", raising=False)
    mmdit.set_ops_for_testing(SW)
    SW.CALLS.clear()
    yield mmdit
    mmdit.set_ops_for_testing(hip_lib)


# ----------------------------------------------------------------------------- the table
def test_default_arguments_give_the_table_from_before(hip_lib):
    from open_sora_amd.mmdit import attention_window_table

    assert attention_window_table(256, 4 * 256, 256, 0, row0=0, n_rows=None).tolist() == [[0, 16], [0, 4], [4, 4], [8, 4], [12, 4]]
    assert attention_window_table(256, 4 * 256, 256, 1, row0=0).tolist() == [[0, 16], [0, 8], [0, 12], [4, 12], [8, 8]]
    for L_txt, N, T, Wf in [(0, 24, 5, 0), (64, 83, 12, 1), (192, 300, 5, 3), (320, 80, 12, 12), (64, 96, 6, 1)]:
        old = attention_window_table(L_txt, N * T, N, Wf)
        assert torch.equal(attention_window_table(L_txt, N * T, N, Wf, row0=0, n_rows=None), old)
        assert torch.equal(attention_window_table(L_txt, N * T, N, Wf, n_rows=L_txt + N * T), old)
    with pytest.raises(TypeError):
        attention_window_table(64, 96, 96, 0, 0, 160)                  # keyword-only
    for bad in (dict(row0=-1), dict(row0=0, n_rows=0), dict(row0=100, n_rows=61), dict(row0=160)):
        with pytest.raises(ValueError):
            attention_window_table(64, 96, 96, 0, **bad)


RANK_GRID = [(L_txt, N, T, Wf, P) for L_txt, N, T in ((64, 96, 6), (64, 83, 12), (192, 300, 5), (128, 24, 40), (0, 80, 12))
             for Wf in (0, 1, 3, 40) for P in (2, 3, 8)]


def test_rank_tables_cover_every_rows_window_and_stay_in_range(hip_lib):
    """every rank of a P = 2 / 3 / 8 split (ceil(L / P) rows, the last rank the rest): its table has one row per 256 of ITS rows, every
    query row's own +-W frames lie inside its block's range, ranges stay inside the image tiles, a block with a text row is full"""
    from open_sora_amd.mmdit import attention_window_table

    ragged = off_tile = mid_block_rank = 0
    for L_txt, N, T, Wf, P in RANK_GRID:
        L_img, L = N * T, L_txt + N * T
        tiles = (L_img + 63) // 64
        Lc = -(-L // P)
        ragged += L % P != 0
        off_tile += N % 64 != 0
        for rank in range(P):
            row0, n_rows = rank * Lc, min((rank + 1) * Lc, L) - rank * Lc
            assert n_rows >= 1
            mid_block_rank += row0 % 256 != 0
            t = attention_window_table(L_txt, L_img, N, Wf, row0=row0, n_rows=n_rows)
            what = (L_txt, N, T, Wf, P, rank)
            assert t.dtype == torch.int32 and t.device.type == "cpu" and tuple(t.shape) == ((n_rows + 255) // 256, 2), what
            first, n = t[:, 0].long(), t[:, 1].long()
            assert bool((first >= 0).all()) and bool((n >= 1).all()) and bool((first + n <= tiles).all()), (what, t)
            for i in range(n_rows):
                blk = i // 256
                a, b = int(first[blk]) * 64, min(int(first[blk] + n[blk]) * 64, L_img)
                if row0 + 256 * blk < L_txt:          # a block with a text row: every tile
                    assert (a, b) == (0, L_img), (what, i)
                    continue
                f = (row0 + i - L_txt) // N
                assert a <= max(0, f - Wf) * N and b >= min(T, f + Wf + 1) * N, (what, i, a, b)
            if Wf >= T:
                assert bool((first == 0).all()) and bool((n == tiles).all()), what
    assert ragged and off_tile and mid_block_rank


def test_rank_tables_are_no_wider_than_the_block_needs(hip_lib):
    """blocks start at row0: with 128-token frames and W = 0 the second rank of L = 256 + 768 over P = 2 (rows 512 ..) sees frames
    2..3 and 4..5 -- and a rank that starts mid-frame sees the frames of ITS blocks, not those of the single-device blocks"""
    from open_sora_amd.mmdit import attention_window_table

    assert attention_window_table(256, 768, 128, 0, row0=512, n_rows=512).tolist() == [[4, 4], [8, 4]]
    assert attention_window_table(256, 768, 128, 0, row0=0, n_rows=512).tolist() == [[0, 12], [0, 4]]
    # row0 = 320 = image row 64: block 0 = image rows 64..319 (frames 0..2), block 1 = image rows 320..383 (frame 2)
    assert attention_window_table(256, 768, 128, 0, row0=320, n_rows=320).tolist() == [[0, 6], [4, 2]]


# ----------------------------------------------------------------------------- the join
@pytest.mark.parametrize("hd", [64, 72, 128])
@pytest.mark.parametrize("n_seg,seg_len,L", [(3, 100, 237), (2, 64, 128), (4, 33, 130), (1, 70, 70)])
def test_join_statement_is_desegment_then_transpose(hd, n_seg, seg_len, L):
    B, H = 2, 2
    D = H * hd
    g = torch.Generator().manual_seed(hd + L)
    wide_k = torch.randn(n_seg, B, seg_len + 3, D + 16, generator=g).to(BF)     # the inputs inside a larger strided buffer
    wide_v = torch.randn(n_seg, B, seg_len + 3, D + 16, generator=g).to(BF)
    k_seg, v_seg = wide_k[:, :, :seg_len, 8: 8 + D], wide_v[:, :, :seg_len, 8: 8 + D]
    last = L - (n_seg - 1) * seg_len
    poison = lambda t: t[-1, :, last:].fill_(float("nan"))                       # rows behind key L - 1: never read
    poison(k_seg), poison(v_seg)
    Lp = (L + 63) // 64 * 64
    k_out, vt_out = torch.full((B, L, D), 7.0, dtype=BF), torch.full((B, H, hd, Lp), 7.0, dtype=BF)
    SW.kv_join(k_seg, v_seg, k_out, vt_out, H, hd, L)
    k_flat = torch.cat([k_seg[s] for s in range(n_seg)], 1)[:, :L].contiguous()
    v_flat = torch.cat([v_seg[s] for s in range(n_seg)], 1)[:, :L].contiguous()
    want_vt = torch.full((B, H, hd, Lp), 3.0, dtype=BF)
    cpu_ops.v_transpose(v_flat, want_vt, H, hd)
    assert torch.equal(k_out.view(torch.int16), k_flat.view(torch.int16))
    assert torch.equal(vt_out.view(torch.int16), want_vt.view(torch.int16))
    for bad in (dict(L=n_seg * seg_len + 1), dict(L=(n_seg - 1) * seg_len)):
        if bad["L"] < 1:
            continue
        with pytest.raises((RuntimeError, IndexError)):
            SW.kv_join(k_seg, v_seg, torch.empty(B, bad["L"], D, dtype=BF), torch.empty(B, H, hd, (bad["L"] + 63) // 64 * 64, dtype=BF), H, hd, bad["L"])


def test_entry_point_is_declared_and_bound(hip_lib):
    with open(os.path.join(ROOT, "include", "osk.h")) as f:
        header = f.read()
    assert "int osk_kv_join_bf16(const void* k_seg, const void* v_seg," in header
    assert "#define OSK_ABI_VERSION 2" in header and hip_lib.lib.osk_abi_version() == 2
    assert len(hip_lib.SIGNATURES["osk_kv_join_bf16"]) == 16
    assert os.path.isfile(os.path.join(ROOT, "open_sora_amd", "csrc", "kv_join.hip"))
    # the binding's own checks raise before anything is launched (CPU tensors: a launch would fault, not raise)
    k = torch.zeros(2, 1, 64, 128, dtype=BF)
    with pytest.raises(AssertionError):
        hip_lib.kv_join(k, k, torch.zeros(1, 128, 128, dtype=BF), torch.zeros(1, 2, 64, 192, dtype=BF), 2, 64, 128)


# ----------------------------------------------------------------------------- the model
_T, _h, _w, _LT = 6, 8, 12, 64                              # 64 text + 6 frames x 96 image tokens = 640 rows
_N = _h * _w


def _model(mmdit, name="hd72_eager_split", **over):
    cfg = dict(configs.GOLDEN[name][0], depth=1, depth_single_blocks=1, **over)
    model = mmdit.Flux(device_map="cpu", torch_dtype=BF, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=BF), strict=True)
    return cfg, model


def _run_sp(model, inp, P, mode, **enable_kw):
    """-> per rank (prediction, the rank's recorded join / window calls, its SeqPar)"""
    from open_sora_amd import seqpar

    def rank_fn(rank, world):
        m = copy.copy(model)
        m.forward = m.forward_ckpt
        object.__setattr__(m, "_osk_ws_cache", {})
        sp = seqpar.enable(m, mode=mode, transport=LocalTransport(world, rank, "cpu"), **enable_kw)
        with torch.inference_mode():
            out = m(**inp).float().clone()
        return out, threading.get_ident(), sp

    SW.CALLS.clear()
    res = run_ranks(P, rank_fn, "cpu")
    return [(out, list(SW.CALLS.get(ident, [])), sp) for out, ident, sp in res]


@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
def test_aligned_split_is_the_single_device_windowed_forward(sw_ops, mode):
    """L_txt 256 + 6 frames x 128 tokens over P = 2: Lc = 512, so a rank's 256-row blocks ARE the single-device blocks and the sharded
    windowed forward computes the single-device windowed forward -- same mask, same CPU arithmetic per row.  Bound: the 2^-7 the
    suite holds a sharded forward to against the single process (tests/test_seqpar_chunked_host.py)."""
    from open_sora_amd.mmdit import attention_window_table

    cfg, model = _model(sw_ops)
    H = cfg["num_heads"]
    inp = torch_inputs(cfg, 1, 6, 8, 16, 256, dtype=BF)
    model.set_attention_window(1, 128)
    with torch.inference_mode():
        single = model(**inp).float().clone()
        off = model.set_attention_window(None)(**inp).float().clone()
    model.set_attention_window(1, 128)
    res = _run_sp(model, inp, 2, mode)
    full = tuple(map(tuple, attention_window_table(256, 768, 128, 1).tolist()))
    for rank, (out, calls, sp) in enumerate(res):
        assert sp.geom == (512, 512) and torch.equal(out, res[0][0])
        joins, wins = [c for c in calls if c[0] == "kv_join"], [c for c in calls if c[0] == "attention_fwd_window"]
        if mode == "allgather":
            assert joins == [("kv_join", 2, 512, 1024, H)] * 2                    # one per block: a double and a single block
            assert len(wins) == 2 and all(c[1:4] == (512, 1024, 256) and c[5] == full[2 * rank: 2 * rank + 2] for c in wins), wins
        else:
            assert joins == [("kv_join", 2, 512, 1024, H // 2)] * 2
            assert len(wins) == 4 and [c[5] for c in wins] == [full[0:2], full[2:4]] * 2 and all(c[1:4] == (512, 1024, 256) for c in wins)
    e, sep = rel_l2(res[0][0], single), rel_l2(off, single)
    print(f"aligned P = 2 {mode}: relL2 sharded vs single-device windowed {e:.3e}; the window moves the forward by {sep:.3e}")
    assert e <= min(2.0 ** -7, sep / 2), (e, sep)


SPLITS = [(2, "allgather", "hd72_eager_split", {}), (2, "ulysses", "hd72_eager_split", {}), (3, "allgather", "hd72_eager_split", {}),
          (3, "ulysses", "hd128_liger_split", dict(hidden_size=384, num_heads=3))]


@pytest.mark.parametrize("P,mode,name,over", SPLITS, ids=[f"P{p}-{m}-{n.split('_')[0]}" for p, m, n, _ in SPLITS])
def test_full_windows_give_the_unwindowed_sharded_forward(sw_ops, P, mode, name, over):
    """L = 64 + 6 x 96 = 640 over P = 2 (Lc = 320: blocks that are not the single-device blocks) and P = 3 (ragged: 214, 214, 212).
    W >= the frame count: every table is full, so the sharded windowed forward sees every key, as the sharded forward without a
    window does; they differ by the merge's second rounding of a row (2^-8 + 2^-9 of its magnitude per block,
    tests/test_attention_window_host.py) -- inside the 2^-7 relL2 of a sharded comparison.  W = 0 must move the result."""
    cfg, model = _model(sw_ops, name, **over)
    H = cfg["num_heads"]
    inp = torch_inputs(cfg, 2, _T, _h, _w, _LT, dtype=BF)
    L, Lc = 640, -(-640 // P)
    plain = _run_sp(model, inp, P, mode)
    assert not any(calls for _, calls, _ in plain)                               # window off: neither a join nor a window call
    model.set_attention_window(_T, _N)
    wide = _run_sp(model, inp, P, mode)
    tiles = (L - _LT + 63) // 64
    for rank, (out, calls, sp) in enumerate(wide):
        assert sp.geom == (Lc, L - (P - 1) * Lc) and torch.equal(out, wide[0][0])
        rows = [L - (P - 1) * Lc if r == P - 1 else Lc for r in range(P)]
        wins = [c for c in calls if c[0] == "attention_fwd_window"]
        assert [c for c in calls if c[0] == "kv_join"] == [("kv_join", P, Lc, L, H if mode == "allgather" else H // P)] * 2
        assert [c[1] for c in wins] == ([rows[rank]] * 2 if mode == "allgather" else rows * 2), wins
        assert all(c[2:4] == (L, _LT) and all(r == (0, tiles) for r in c[5]) and len(c[5]) == (c[1] + 255) // 256 for c in wins)
    e = rel_l2(wide[0][0], plain[0][0])
    model.set_attention_window(0, _N)
    narrow = _run_sp(model, inp, P, mode)
    e0 = rel_l2(narrow[0][0], plain[0][0])
    print(f"P = {P} {mode} {name}: relL2 full windows vs no window {e:.3e}; W = 0 vs no window {e0:.3e}")
    assert e <= 2.0 ** -7 and e0 > 2 * e, (e, e0)


def test_what_stays_refused_under_sequence_parallelism(sw_ops):
    from open_sora_amd import seqpar
    from tests.local_transport import LocalWorld

    cfg, model = _model(sw_ops)
    tp = lambda: LocalTransport(LocalWorld(2), 0, "cpu")
    inp = torch_inputs(cfg, 1, _T, _h, _w, _LT, dtype=BF)
    # bf16, both orders: accepted
    seqpar.enable(model, mode="allgather", transport=tp())
    assert model.set_attention_window(1, _N)._attn_window == (1, _N)
    model.set_attention_window(None)
    seqpar.disable(model)
    model.set_attention_window(1, _N)
    sp = seqpar.enable(model, mode="allgather", transport=tp())
    assert model._window_table(_LT, _T * _N, sp) is not None
    # fp8, every order
    with pytest.raises(ValueError, match="fp8"):
        model.enable_fp8(True)
    model.set_attention_window(None)
    model.enable_fp8(True)
    with pytest.raises(ValueError, match="fp8"):
        model.set_attention_window(1, _N)
    seqpar.disable(model)
    sw_ops.set_ops_for_testing(types.SimpleNamespace(**dict(vars(SW), attention_fwd_window_fp8=None)))   # a table with the fp8 window entry
    model.set_attention_window(1, _N)                                            # single device: fp8 + window is fine there
    seqpar.enable(model, mode="allgather", transport=tp())
    with torch.inference_mode(), pytest.raises(ValueError, match="fp8"):
        model(**inp)
    sw_ops.set_ops_for_testing(SW)
    model.enable_fp8(False)
    # kv_chunks > 1, both orders
    seqpar.enable(model, mode="allgather", transport=tp(), kv_chunks=2)
    with torch.inference_mode(), pytest.raises(ValueError, match="kv_chunks"):
        model(**inp)
    model.set_attention_window(None)
    with pytest.raises(ValueError, match="kv_chunks"):
        model.set_attention_window(1, _N)
    # the step cache stays out of scope for a sharded model
    seqpar.enable(model, mode="allgather", transport=tp())
    model.set_attention_window(1, _N)
    with pytest.raises(ValueError, match="step_cache"):
        model.step_cache_begin(1, 3, _T * _N, "cpu")
    # a text length that is no multiple of 64: refused by the forward that sees it, before any launch or exchange
    with torch.inference_mode(), pytest.raises(ValueError, match="multiple of 64"):
        model(**torch_inputs(cfg, 1, _T, _h, _w, 40, dtype=BF))
    # an sp object from before the window path keeps its refusal
    model._sp = types.SimpleNamespace(shard_range=lambda L, L_txt: None)
    with pytest.raises(ValueError, match="sequence parallelism"):
        model.set_attention_window(1, _N)
    assert not SW.CALLS
