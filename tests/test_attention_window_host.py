"""CPU: the host side of opt-in frame-window attention -- the table of mmdit.attention_window_table, the binding's validation of a
table, MMDiTModel.set_attention_window and its refusals, a small MMDiT on the CPU statement of osk_attention_fwd_window_bf16
(tests/cpu_ops_window.py), the sampler's attn_window_frames keyword -- and, before a GPU is involved, that the f64 reference and
derived tolerance of tests/cpu_ops_window.py hold for a torch emulation of the two launches and the merge and reject a table that
is off by one tile and a prefix that never reaches the merge (the practice of tests/test_attention_refs.py).  The kernels
themselves are checked on the GPU by tests/test_gpu_attention_window.py."""
import functools
import os
import types

import pytest
import torch

from oracle import configs, sampling_oracle as S
from tests import cpu_ops_window as W
from tests.util import rel_l2, torch_inputs, torch_params

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def window_ops(hip_lib, monkeypatch):
    from open_sora_amd import mmdit

    monkeypatch.delenv("OSK_ATTN_WINDOW_FRAMES", raising=False)
    mmdit.set_ops_for_testing(W)
    W.WINDOW_CALLS.clear()
    yield mmdit
    mmdit.set_ops_for_testing(hip_lib)


# ----------------------------------------------------------------------------- the table
GRID = [(L_txt, N, T, Wf) for L_txt in (0, 64, 192, 320) for N in (24, 64, 80, 83, 300) for T in (1, 5, 12) for Wf in (0, 1, 3, 12)]


def test_table_covers_every_rows_window_and_stays_in_range(hip_lib):
    from open_sora_amd.mmdit import attention_window_table

    partial_blocks = off_tile_frames = 0
    for L_txt, N, T, Wf in GRID:
        L_img, L = N * T, L_txt + N * T
        tiles = (L_img + 63) // 64
        t = attention_window_table(L_txt, L_img, N, Wf)
        assert t.dtype == torch.int32 and t.device.type == "cpu" and tuple(t.shape) == ((L + 255) // 256, 2)
        first, n = t[:, 0].long(), t[:, 1].long()
        assert bool((first >= 0).all()) and bool((n >= 1).all()) and bool((first + n <= tiles).all()), (L_txt, N, T, Wf, t)
        partial_blocks += L % 256 != 0
        off_tile_frames += N % 64 != 0
        for r in range(L):
            a, b = int(first[r // 256]) * 64, min(int(first[r // 256] + n[r // 256]) * 64, L_img)
            if 256 * (r // 256) < L_txt:          # a block with a text row: every tile
                assert (a, b) == (0, L_img), (L_txt, N, T, Wf, r)
                continue
            f = (r - L_txt) // N
            assert a <= max(0, f - Wf) * N and b >= min(T, f + Wf + 1) * N, (L_txt, N, T, Wf, r, a, b)
        if Wf >= T:
            assert bool((first == 0).all()) and bool((n == tiles).all())
    assert partial_blocks and off_tile_frames


def test_table_is_no_wider_than_the_block_needs(hip_lib):
    """the range of an image block is exactly its frames' +-W window rounded outward to tiles: W = 0 at tile-aligned frames of 256
    tokens is the block's own frame, nothing else"""
    from open_sora_amd.mmdit import attention_window_table, window_tile_fraction

    t = attention_window_table(256, 4 * 256, 256, 0)
    assert t.tolist() == [[0, 16], [0, 4], [4, 4], [8, 4], [12, 4]]
    assert attention_window_table(256, 4 * 256, 256, 1).tolist() == [[0, 16], [0, 8], [0, 12], [4, 12], [8, 8]]
    assert window_tile_fraction(t, 256, 1024) == pytest.approx((20 + 4 * 8) / (5 * 20))
    for bad in [(-1, 64, 64, 0), (0, 0, 64, 0), (0, 100, 64, 0), (0, 64, 0, 0), (0, 64, 64, -1)]:
        with pytest.raises(ValueError):
            attention_window_table(*bad)


# ----------------------------------------------------------------------------- the binding's validation (no GPU: it raises first)
def test_binding_refuses_bad_tables(hip_lib):
    Lq = Lk = 64 + 960                                  # 4 query blocks, 15 body tiles
    good = torch.tensor([[0, 15], [0, 1], [14, 1], [3, 2]], dtype=torch.int32)
    hip_lib.check_window_table(good, Lq, Lk, 64)
    bad = {
        "shape": good[:3], "one_dim": good.reshape(-1), "dtype": good.long(), "negative_first": torch.tensor([[0, 15], [-1, 2], [14, 1], [3, 2]], dtype=torch.int32),
        "empty_range": torch.tensor([[0, 15], [0, 0], [14, 1], [3, 2]], dtype=torch.int32),
        "past_the_end": torch.tensor([[0, 15], [0, 1], [14, 2], [3, 2]], dtype=torch.int32),
        "first_past_the_end": torch.tensor([[0, 15], [0, 1], [15, 1], [3, 2]], dtype=torch.int32),
    }
    for name, t in bad.items():
        with pytest.raises(ValueError):
            hip_lib.check_window_table(t, Lq, Lk, 64)
        print("refused:", name)
    for n_prefix in (32, -64, Lk):
        with pytest.raises(ValueError):
            hip_lib.check_window_table(good, Lq, Lk, n_prefix)
    # the call itself raises before anything is launched (CPU tensors: a launch would fault, not raise ValueError)
    q = torch.zeros(1, Lq, 128, dtype=BF)
    vt = torch.zeros(1, 2, 64, Lk, dtype=BF)
    with pytest.raises(ValueError):
        hip_lib.attention_fwd_window(q, q, vt, torch.empty_like(q), 2, 64, 0.125, n_prefix=64, windows=bad["past_the_end"])


def test_entry_points_are_declared_and_bound(hip_lib):
    with open(os.path.join(ROOT, "include", "osk.h")) as f:
        header = f.read()
    assert "int64_t osk_attention_window_workspace_bytes(int B, int H, int Lq, int hd);" in header
    assert "int osk_attention_fwd_window_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride," in header
    assert "#define OSK_ABI_VERSION 2" in header and hip_lib.lib.osk_abi_version() == 2
    assert len(hip_lib.SIGNATURES["osk_attention_fwd_window_bf16"]) == 26 and len(hip_lib.SIGNATURES["osk_attention_window_workspace_bytes"]) == 4
    need = hip_lib.attention_window_workspace_bytes(2, 3, 300, 72)
    assert need >= 2 * 2 * 3 * 256 * 73 * 4 + 2 * 3 * 300 * 4 and need % 16 == 0


# ----------------------------------------------------------------------------- reference, tolerance, emulation, mutants
H_, B_ = 2, 2
CASES = [(hd, body, Bkv, table) for hd in (64, 72, 128) for body, Bkv in ((960, 1), (996, 2)) for table in ("w0", "w1", "hand")]


def make_table(name: str, n_prefix: int, body: int) -> torch.Tensor:
    from open_sora_amd.mmdit import attention_window_table

    if name == "hand":
        return W.hand_table(n_prefix + body, body)
    return attention_window_table(n_prefix, body, body // 12, int(name[1:]))


@functools.lru_cache(maxsize=None)
def case(hd: int, body: int, Bkv: int, table: str, n_prefix: int = 64):
    q, k, v, sb = W.operands(hd, H_, B_, Bkv, n_prefix + body)
    t = make_table(table, n_prefix, body)
    return q, k, v, sb, t, W.reference(q, k, v, H_, hd, n_prefix, t)


@pytest.mark.parametrize("hd,body,Bkv,table", CASES)
def test_emulation_stays_inside_the_derived_tolerance(hip_lib, hd, body, Bkv, table):
    q, k, v, sb, t, ref = case(hd, body, Bkv, table)
    worst = [0.0, 0.0]
    for mode in ("max", "max-8", sb):                        # the general body's two ends, the FAST body
        out, lse = W.emulate(q, k, v, H_, hd, 64, t, mode)
        r = W.R.ratios(out, lse, ref)
        worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    print(f"window emulation hd {hd} body {body} Bkv {Bkv} {table}: err/tol {worst[0]:.3f}  dlse/tol {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst


@pytest.mark.parametrize("hd,body,Bkv,table", [c for c in CASES if c[0] == 72])
def test_emulation_mutants_leave_the_tolerance(hip_lib, hd, body, Bkv, table):
    """a table shifted by one tile and a prefix that never reaches the merge each put at least one row outside the tolerance"""
    q, k, v, sb, t, ref = case(hd, body, Bkv, table)
    tiles = (body + 63) // 64
    shifted = t.clone()
    movable = (t[:, 1] < tiles)                              # a full range has nowhere to go
    assert bool(movable.any())
    up = movable & (t[:, 0] + t[:, 1] < tiles)
    shifted[:, 0] += torch.where(up, 1, torch.where(movable, -1, 0)).to(torch.int32)
    for what, kw, tab in (("table shifted by one tile", {}, shifted), ("prefix dropped from the merge", dict(drop_prefix=True), t)):
        out, lse = W.emulate(q, k, v, H_, hd, 64, tab, "max", **kw)
        bad_rows = ((out.double() - ref["out"]).abs() > ref["tol"]).any(-1)
        print(f"{what}: {int(bad_rows.sum())} of {bad_rows.numel()} rows leave the tolerance")
        assert bool(bad_rows.any()), what
        if not kw:                                           # every block whose range moved is caught
            for i in torch.nonzero(movable).flatten().tolist():
                assert bool(bad_rows[:, :, 256 * i: 256 * (i + 1)].any()), (what, i)


def test_cpu_statement_agrees_with_the_reference(hip_lib):
    q, k, v, sb, t, ref = case(72, 996, 2, "hand")
    Lk = k.shape[1]
    vt = torch.zeros(2, H_, 72, (Lk + 63) // 64 * 64, dtype=BF)
    W.v_transpose(v, vt, H_, 72)
    out, lse = torch.empty_like(q), torch.empty(B_, H_, q.shape[1])
    W.attention_fwd_window(q, k, vt, out, H_, 72, 72 ** -0.5, n_prefix=64, windows=t, lse=lse, q_prescaled=True, score_bound=sb,
                           workspace=W.attention_window_workspace(B_, H_, q.shape[1], 72, "cpu"))
    r = W.R.ratios(W.R.heads(out.float(), H_, 72), lse, ref)
    assert r[0] <= 1.0 and r[1] <= 1.0, r


# ----------------------------------------------------------------------------- the model
_T, _h, _w, _LT = 6, 8, 12, 64                              # 64 text + 6 frames x 96 image tokens: 3 query blocks
_N = _h * _w


def _model(mmdit, name="hd64_eager_fused"):
    cfg = dict(configs.GOLDEN[name][0], depth=1, depth_single_blocks=1)
    model = mmdit.Flux(device_map="cpu", torch_dtype=BF, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=BF), strict=True)
    return cfg, model


def _brute_force_mask(L_txt, N, T, Wf):
    """the mask the feature states, from sets of rows and keys: a row sees the text, and of the image the tiles touched by the +-W
    frames of ANY image row of its 256-row block; a block with a text row sees everything"""
    L = L_txt + N * T
    m = torch.zeros(L, L, dtype=torch.bool)
    m[:, :L_txt] = True
    for r0 in range(0, L, 256):
        rows = range(r0, min(r0 + 256, L))
        if r0 < L_txt:
            m[r0: r0 + 256] = True
            continue
        tiles = set()
        for r in rows:
            f = (r - L_txt) // N
            for key in range(max(0, f - Wf) * N, min(T, f + Wf + 1) * N):
                tiles.add(key // 64)
        for tile in tiles:
            m[r0: r0 + 256, L_txt + 64 * tile: min(L_txt + 64 * tile + 64, L)] = True
    return m


def test_windowed_forward_on_the_cpu_ops(window_ops):
    cfg, model = _model(window_ops)
    x = torch_inputs(cfg, 1, _T, _h, _w, _LT, dtype=BF)
    assert x["img"].shape[1] == _T * _N and x["txt"].shape[1] == _LT
    with torch.inference_mode():
        full = model(**x).float().clone()
        assert not W.WINDOW_CALLS and model.attention_report()["attention_window"] is None
        model.set_attention_window(_T, _N)
        wide = model(**x).float().clone()
        calls = len(W.WINDOW_CALLS)
        assert calls == 2 and all(c[0] == _LT for c in W.WINDOW_CALLS)           # one double block, one single block
        rep = model.attention_report()["attention_window"]
        assert rep == {"window_frames": _T, "frame_tokens": _N, "visited_tile_fraction": 1.0}
        model.set_attention_window(0, _N)
        narrow = model(**x).float().clone()
        # blocks: [text + frames 0..1] all 9 image tiles; [frames 2..4] tiles 3..7; [frames 4..5] tiles 6..8; + the text tile each
        assert model.attention_report()["attention_window"]["visited_tile_fraction"] == pytest.approx((10 + 6 + 4) / 30)
        # the same forward with the attention as a dense masked softmax in torch, the mask built from sets
        mask = _brute_force_mask(_LT, _N, _T, 0)

        def dense(q, k, vt, out, H, hd, scale, *, n_prefix, windows, lse=None, q_prescaled=False, kv_batches=0, score_bound=0.0,
                  workspace=None):
            B, L, D = q.shape
            v = torch.empty(B, L, D, dtype=BF)
            Lp = vt.shape[-1]
            v.copy_(vt.float()[..., torch.argsort(W.pos2key(hd, Lp))][..., :L].permute(0, 3, 1, 2).reshape(B, L, D))
            hs = lambda t: t.float().reshape(B, L, H, hd).permute(0, 2, 1, 3)
            s = hs(q) @ hs(k).transpose(-1, -2) * 0.6931471805599453
            o = torch.softmax(s.masked_fill(~mask, float("-inf")), -1) @ hs(v)
            out.copy_(o.permute(0, 2, 1, 3).reshape(B, L, D).to(BF))

        window_ops.set_ops_for_testing(types.SimpleNamespace(**dict(vars(W), attention_fwd_window=dense)))
        masked = model(**x).float().clone()
        window_ops.set_ops_for_testing(W)
        model.set_attention_window(None)
        again = model(**x).float().clone()
    assert len(W.WINDOW_CALLS) == 2 * calls and torch.equal(again, full)          # off: the path from before, launch for launch
    # W = T: every range full -- the merge tolerance (two roundings of a row instead of one: 2^-8 + 2^-9 of its magnitude)
    assert (wide - full).abs().max() <= (2.0 ** -8 + 2.0 ** -9) * full.abs().max(), (wide - full).abs().max()
    # W = 0: the mask is felt, and it is the mask the feature states
    print(f"W = 0 vs unwindowed: relL2 {rel_l2(narrow, full):.3e}; vs the dense masked forward: {rel_l2(narrow, masked):.3e}")
    assert rel_l2(narrow, full) > 1e-2
    assert torch.allclose(narrow, masked, rtol=2.0 ** -7, atol=2.0 ** -8 * float(full.abs().max()))


def test_table_follows_the_geometry(window_ops):
    cfg, model = _model(window_ops)
    model.set_attention_window(1, _N)
    with torch.inference_mode():
        model(**torch_inputs(cfg, 1, _T, _h, _w, _LT, dtype=BF))
        first = W.WINDOW_CALLS[-1][2]
        model(**torch_inputs(cfg, 1, 3, _h, _w, _LT, dtype=BF))
    assert len(first) == 3 and len(W.WINDOW_CALLS[-1][2]) == 2 and W.WINDOW_CALLS[-1][2] != first[:2]
    assert "_attn_window" not in model.state_dict() and not any("window" in k_ for k_ in model.state_dict())


def test_set_attention_window_refusals(window_ops, monkeypatch):
    cfg, model = _model(window_ops, "hd72_eager_split")
    with pytest.raises(ValueError, match="frame_tokens"):
        model.set_attention_window(2)
    with pytest.raises(ValueError):
        model.set_attention_window(-1, 96)
    assert model.set_attention_window()._attn_window is None                     # no argument, no environment: off
    monkeypatch.setenv("OSK_ATTN_WINDOW_FRAMES", "3")
    assert model.set_attention_window(frame_tokens=96)._attn_window == (3, 96)    # the environment's default
    assert model.set_attention_window(None)._attn_window is None
    # fp8, both orders
    model.enable_fp8(True)
    with pytest.raises(ValueError, match="fp8"):
        model.set_attention_window(1, 96)
    model.enable_fp8(False)
    model.set_attention_window(1, 96)
    with pytest.raises(ValueError, match="fp8"):
        model.enable_fp8(True)
    # a text length that is no multiple of 64: refused by the forward that sees it, before any launch
    x = torch_inputs(cfg, 1, 2, 8, 12, 40, dtype=BF)
    with torch.inference_mode(), pytest.raises(ValueError, match="multiple of 64"):
        model(**x)
    assert not W.WINDOW_CALLS
    # sequence parallelism, both orders
    model.set_attention_window(None)
    sp = types.SimpleNamespace(shard_range=lambda L, L_txt: None)    # what seqpar.enable leaves on the model: any object
    model._sp = sp
    with pytest.raises(ValueError, match="sequence parallelism"):
        model.set_attention_window(1, 96)
    model._sp = None
    model.set_attention_window(1, 96)
    model._sp = sp
    with torch.inference_mode(), pytest.raises(ValueError, match="sequence parallelism"):
        model(**torch_inputs(cfg, 1, 2, 8, 12, 64, dtype=BF))


# ----------------------------------------------------------------------------- the sampler
def test_denoise_sets_the_window_for_the_loop_and_restores_it(window_ops):
    from open_sora_amd import sampling

    cfg, model = _model(window_ops)
    n, T, Hh, Ww, Lt = 1, 3, 16, 24, 64                      # 96 tokens per latent frame at patch size 2
    g = torch.Generator().manual_seed(7)
    z = torch.randn(n, 16, T, Hh, Ww, generator=g).to(BF)
    masks = torch.zeros(n, 1, T, Hh, Ww, dtype=BF)
    masks[:, :, 0] = 1
    masked_ref = (torch.randn(n, 16, T, Hh, Ww, generator=g) * masks.float()).to(BF)
    txt = (torch.randn(3 * n, Lt, cfg["context_in_dim"], generator=g) * 0.2).to(BF)
    y_vec = torch.randn(3 * n, cfg["vec_in_dim"], generator=g).to(BF)
    img_ids, txt_ids = S.grid_ids(3 * n, T, Hh // 2, Ww // 2, Lt, torch.float32)
    args = dict(img=S.pack(z.float()).to(BF).repeat(3, 1, 1), masks=masks, masked_ref=masked_ref, img_ids=img_ids.to(BF), txt=txt,
                txt_ids=txt_ids.to(BF), y_vec=y_vec, timesteps=sampling.get_schedule(3, 96, T), guidance=7.5, guidance_img=3.0)
    den = sampling.I2VDenoiser()
    with torch.inference_mode():
        plain = den.denoise(model, **dict(args))
        assert not W.WINDOW_CALLS and model._attn_window is None
        windowed = den.denoise(model, attn_window_frames=0, **dict(args))
        assert model._attn_window is None and len(W.WINDOW_CALLS) == 3 * 2       # three steps, two blocks
        want = tuple(map(tuple, window_ops.attention_window_table(Lt, T * 96, 96, 0).tolist()))
        assert all(c[2] == want for c in W.WINDOW_CALLS)
        assert not torch.equal(plain, windowed)
        # a previous setting comes back, also under cfg_prune and after a loop that raises
        model.set_attention_window(2, 96)
        den.denoise(model, attn_window_frames=1, cfg_prune=True, **dict(args))
        assert model._attn_window == (2, 96)
        with pytest.raises(TypeError):
            den.denoise(model, attn_window_frames=1, **{k_: v_ for k_, v_ in args.items() if k_ != "txt"})
        assert model._attn_window == (2, 96)
        # explicit None: off for this loop whatever the model was set to?  No: None leaves the model's own setting alone
        W.WINDOW_CALLS.clear()
        den.denoise(model, attn_window_frames=None, **dict(args))
        assert W.WINDOW_CALLS and model._attn_window == (2, 96)
