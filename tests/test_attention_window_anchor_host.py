"""CPU: frame-window attention with anchor frames -- the host layers.  The bounds and the table (every row's own frames +- W, the
anchor frames and the text inside its block's stated key set; the three parts disjoint and tile-aligned; (0, 0) the table from
before; no body refused), the CPU statement against the f64 reference and its mutants, the declarations and the binding, the calls
the model makes in bf16 / pv8 / qk8 mode on a substituted kernel table, the "cond" derivation from the sampler's masks, and the
sharded forward with ranks as threads in both exchange modes."""
import copy
import os
import threading

import pytest
import torch

from oracle import sampling_oracle as S
from tests import cpu_ops_window_anchor as A
from tests.local_transport import LocalTransport, run_ranks
from tests.test_attention_window_fp8_host import MODELS, _N, _T, _LT, build, model_case
from tests.test_attention_window_host import _model
from tests.test_seqpar_window_host import _model as _sp_model
from tests.util import rel_l2, torch_inputs

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = A.R


@pytest.fixture()
def anchor_ops(hip_lib, monkeypatch):
    from open_sora_amd import mmdit

    for name in ("OSK_ATTN_WINDOW_FRAMES", "OSK_ATTN_WINDOW_ANCHORS", "OSK_SP_KV_CHUNKS"):
        monkeypatch.delenv(name, raising=False)
    mmdit.set_ops_for_testing(A)
    A.ANCHOR_CALLS.clear(), A.WINDOW_CALLS.clear(), A.WINDOW_FP8_CALLS.clear()
    yield mmdit
    mmdit.set_ops_for_testing(hip_lib)


# ----------------------------------------------------------------------------- bounds and table
GEOMS = [(64, 96, 6), (64, 83, 12), (128, 24, 40), (192, 300, 5), (0, 64, 7), (320, 80, 5)]
GRID = [(L_txt, N, T, Wf, a, b) for L_txt, N, T in GEOMS for Wf in (0, 1, 3) for a, b in ((1, 0), (0, 1), (1, 1), (2, 1), (0, 2))]


def test_bounds_are_tile_aligned_supersets(hip_lib):
    from open_sora_amd.mmdit import attention_window_bounds

    assert attention_window_bounds(64, 576, 96, 1, 0) == (192, 0)
    assert attention_window_bounds(64, 576, 96, 0, 1) == (64, 128)
    assert attention_window_bounds(64, 576, 96, 1, 1) == (192, 128)
    assert attention_window_bounds(128, 640, 128, 1, 1) == (256, 128)
    assert attention_window_bounds(100, 576, 96, 0, 0) == (100, 0)          # no anchors: L_txt as it is, whatever it is
    for L_txt, N, T in GEOMS:
        L = L_txt + N * T
        for a in range(0, T):
            for b in range(0, T - a):
                try:
                    n_prefix, n_suffix = attention_window_bounds(L_txt, N * T, N, a, b)
                except ValueError:
                    s0 = (L - b * N) // 64 * 64 if b else L
                    assert s0 <= (L_txt + a * N + 63) // 64 * 64, (L_txt, N, T, a, b)
                    continue
                if (a, b) == (0, 0):
                    continue
                s0 = L - n_suffix
                assert n_prefix % 64 == 0 and 0 <= n_prefix - (L_txt + a * N) < 64
                assert (n_suffix == 0) == (b == 0) and (b == 0 or (s0 % 64 == 0 and 0 <= (L - b * N) - s0 < 64)) and n_prefix < s0


def test_anchors_that_leave_no_body_are_refused(hip_lib):
    from open_sora_amd.mmdit import attention_window_bounds, attention_window_table

    for args in ((64, 576, 96, 6, 0), (64, 576, 96, 3, 3), (64, 576, 96, 0, 6), (64, 192, 96, 1, 1), (0, 64, 64, 1, 0)):
        with pytest.raises(ValueError):
            attention_window_bounds(*args)
        with pytest.raises(ValueError):
            attention_window_table(args[0], args[1], args[2], 0, anchor_head=args[3], anchor_tail=args[4])
    with pytest.raises(ValueError):
        attention_window_bounds(64, 576, 96, -1, 0)


def test_table_covers_window_anchors_and_text_in_three_disjoint_aligned_parts(hip_lib):
    from open_sora_amd.mmdit import attention_window_bounds, attention_window_table

    clipped_to_one = inside_run = 0
    for L_txt, N, T, Wf, a, b in GRID:
        L_img, L = N * T, L_txt + N * T
        try:
            n_prefix, n_suffix = attention_window_bounds(L_txt, L_img, N, a, b)
        except ValueError:
            continue
        s0 = L - n_suffix
        body = (s0 - n_prefix + 63) // 64
        for row0, n_rows in ((0, L), (100, L - 100), (L // 3, L // 3 + 1)):
            t = attention_window_table(L_txt, L_img, N, Wf, row0=row0, n_rows=n_rows, anchor_head=a, anchor_tail=b)
            assert t.dtype == torch.int32 and tuple(t.shape) == ((n_rows + 255) // 256, 2)
            first, n = t[:, 0].long(), t[:, 1].long()
            assert bool((first >= 0).all()) and bool((n >= 1).all()) and bool((first + n <= body).all()), (L_txt, N, T, Wf, a, b, t)
            for i in range(t.shape[0]):
                pre, run, suf = A.anchor_key_sets(n_prefix, n_suffix, L, int(first[i]), int(n[i]))
                # disjoint, tile-aligned: the prefix ends and the run starts on tiles of the whole key axis, the suffix starts on one
                assert len(pre) == n_prefix and n_prefix % 64 == 0 and int(run[0]) % 64 == 0 and int(run[0]) >= n_prefix
                assert int(run[-1]) < s0 and (n_suffix == 0 or (s0 % 64 == 0 and int(suf[0]) == s0 and int(suf[-1]) == L - 1))
                assert (int(run[-1]) + 1) % 64 == 0 or int(run[-1]) + 1 == s0 == L
                seen = torch.zeros(L, dtype=torch.bool)
                seen[torch.cat([pre, run, suf])] = True
                # text and anchor frames
                assert bool(seen[:L_txt + a * N].all()) and bool(seen[L - b * N:].all())
                r_lo, r_hi = row0 + 256 * i, min(row0 + 256 * (i + 1), row0 + n_rows)
                if r_lo < L_txt:
                    assert bool(seen.all()), "a block with a text row keeps every key"
                    continue
                for r in (r_lo, r_hi - 1, (r_lo + r_hi) // 2):
                    f = (r - L_txt) // N
                    assert bool(seen[L_txt + max(0, f - Wf) * N: L_txt + min(T, f + Wf + 1) * N].all()), (L_txt, N, T, Wf, a, b, row0, r)
                f0, f1 = (r_lo - L_txt) // N, (r_hi - 1 - L_txt) // N
                k0, k1 = L_txt + max(0, f0 - Wf) * N, L_txt + min(T, f1 + Wf + 1) * N
                if k1 <= n_prefix or k0 >= s0:
                    clipped_to_one += 1
                    assert int(n[i]) == 1 and int(first[i]) == (0 if k1 <= n_prefix else body - 1)
                else:
                    inside_run += 1
                    # no wider than the rule: the run rounded outward, clipped to the body
                    assert int(run[0]) == max(n_prefix, k0 // 64 * 64) and int(run[-1]) + 1 == min(s0, (k1 + 63) // 64 * 64)
    assert clipped_to_one and inside_run


def test_without_anchors_table_and_prefix_are_those_from_before(hip_lib):
    from open_sora_amd.mmdit import attention_window_bounds, attention_window_table

    for L_txt, N, T in GEOMS:
        for Wf in (0, 1, 3):
            for kw in ({}, dict(row0=77, n_rows=N * T - 100)):
                assert torch.equal(attention_window_table(L_txt, N * T, N, Wf, anchor_head=0, anchor_tail=0, **kw),
                                   attention_window_table(L_txt, N * T, N, Wf, **kw))
        assert attention_window_bounds(L_txt, N * T, N, 0, 0) == (L_txt, 0)


# ----------------------------------------------------------------------------- declarations and binding
def test_entry_points_are_declared_and_bound(hip_lib):
    with open(os.path.join(ROOT, "include", "osk.h")) as f:
        header = f.read()
    assert "int64_t osk_attention_window_anchor_workspace_bytes(int B, int H, int Lq, int hd);" in header
    assert "int osk_attention_fwd_window_anchor_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride," in header
    assert "int osk_attention_merge_into2_bf16(void* out, int64_t o_batch_stride, int64_t o_row_stride, float* lse, const float* o_b," in header
    assert "#define OSK_ABI_VERSION 2" in header and hip_lib.lib.osk_abi_version() == 2
    assert len(hip_lib.SIGNATURES["osk_attention_fwd_window_anchor_bf16"]) == 30 and len(hip_lib.SIGNATURES["osk_attention_merge_into2_bf16"]) == 13
    for name in ("attention_fwd_window_anchor", "attention_merge_into2", "attention_window_anchor_workspace_bytes"):
        assert callable(getattr(hip_lib, name))
    one, two = hip_lib.attention_window_workspace_bytes(2, 3, 300, 72), hip_lib.attention_window_anchor_workspace_bytes(2, 3, 300, 72)
    lse = (2 * 3 * 300 * 4 + 15) // 16 * 16
    assert two == 2 * (one - lse) + lse and two % 16 == 0
    t = torch.tensor([[0, 2]] * 2, dtype=torch.int32)
    hip_lib.check_window_table(t, 300, 512, 64, 128)
    for bad in ((64, 100), (64, -64), (256, 256), (320, 256)):
        with pytest.raises(ValueError):
            hip_lib.check_window_table(t, 300, 512, *bad)
    with pytest.raises(ValueError):
        hip_lib.check_window_table(torch.tensor([[0, 6]] * 2, dtype=torch.int32), 300, 512, 64, 128)      # the body has 5 tiles


# ----------------------------------------------------------------------------- the CPU statement, the reference, mutants
H_, B_ = 2, 2


@pytest.mark.parametrize("kind,hd", [("bf16", 64), ("bf16", 72), ("pv8", 72), ("qk8", 128)])
def test_cpu_statement_holds_and_its_mutants_leave_the_tolerance(hip_lib, kind, hd):
    """64 + 6 x 96 keys, anchors (1, 1), W = 0, a query slice that starts off the block grid.  The statement with the stated
    arguments stays inside the derived tolerance; with one table row moved by a tile, or the suffix 64 keys short, it does not --
    so the tolerance tells the masks apart."""
    from open_sora_amd.mmdit import attention_window_bounds, attention_window_table
    from tests.test_attention_window_fp8_host import packed

    L_txt, N, T = 64, 96, 6
    L = L_txt + N * T
    q, k, v, sb = A.operands(hd, H_, B_, B_, L)
    q = q[:, 100:].contiguous()
    n_prefix, n_suffix = attention_window_bounds(L_txt, N * T, N, 1, 1)
    t = attention_window_table(L_txt, N * T, N, 0, row0=100, n_rows=L - 100, anchor_head=1, anchor_tail=1)
    ref = A.reference3(q, k, v, H_, hd, n_prefix, n_suffix, t, kind)
    if kind == "bf16":
        vt = torch.zeros(B_, H_, hd, L, dtype=BF)
        A.v_transpose(v, vt, H_, hd)
        kk, kw = k, {}
    else:
        kk, sk, vt, sv = packed(A, k, v, hd, kind)
        kw = dict(k_scale=sk, v_scale=sv, Lk=L)
    ws = A.attention_window_anchor_workspace(B_, H_, q.shape[1], hd, "cpu")

    def run(table, suffix):
        out, lse = torch.empty_like(q), torch.empty(B_, H_, q.shape[1])
        A.attention_fwd_window_anchor(q, kk, vt, out, H_, hd, hd ** -0.5, n_prefix=n_prefix, n_suffix=suffix, windows=table, mode=kind, lse=lse,
                                      q_prescaled=True, workspace=ws, **kw)
        return R.ratios(R.heads(out.float(), H_, hd), lse, ref)

    good = run(t, n_suffix)
    moved = t.clone()
    moved[1, 0] += 1 if int(moved[1, 0] + moved[1, 1]) < (L - n_suffix - n_prefix) // 64 else -1
    off_by_one, short = run(moved, n_suffix), run(t, n_suffix - 64)
    print(f"{kind} hd {hd}: statement err/tol {good[0]:.3f} dlse/tol {good[1]:.3f}; table off by one tile {off_by_one[0]:.1f} / {off_by_one[1]:.1f}; "
          f"suffix 64 keys short {short[0]:.1f} / {short[1]:.1f}")
    assert max(good) <= 1.0 and max(off_by_one) > 1.0 and max(short) > 1.0


def test_three_part_merge_statement(hip_lib):
    g = torch.Generator().manual_seed(3)
    B, H, Lq, hd = 1, 2, 20, 64
    out = torch.randn(B, Lq, H * hd, generator=g).to(BF)
    lse = torch.randn(3, B, H, 256, generator=g)
    lse[0, :, :, 0], lse[1, :, :, 0:2], lse[2, :, :, 0:3] = float("-inf"), float("-inf"), float("-inf")
    o = torch.randn(2, B, H, 256, hd, generator=g)
    la = lse[0, :, :, :Lq].contiguous()
    want, wl = A.merge3_f64(out, la, o[0], lse[1], o[1], lse[2], H, hd)
    got = A.attention_merge_into2(out.clone(), la, o[0], lse[1], o[1], lse[2], H, hd)
    assert bool((got[:, 0] == 0).all()) and bool(torch.isinf(la[:, :, 0]).all()) and torch.isfinite(got.float()).all()
    assert torch.equal(got[:, 1], out[:, 1])                              # row 1: the finished row alone, weight 1
    assert bool(((got.double() - want).abs() <= 2.0 ** -8 * want.abs() + 1e-30).all()) and torch.allclose(la.double()[:, :, 3:], wl[:, :, 3:], atol=1e-6)


# ----------------------------------------------------------------------------- the model's calls
def test_bf16_model_calls_the_anchor_entry_and_the_old_entries_without_anchors(anchor_ops):
    mmdit = anchor_ops
    cfg, model = _model(mmdit)
    inp = torch_inputs(cfg, 1, _T, 8, 12, _LT, dtype=BF)
    with torch.inference_mode():
        off = model(**inp).float().clone()
        narrow = model.set_attention_window(0, _N)(**inp).float().clone()
        assert not A.anchor_calls() and len(A.WINDOW_CALLS) == 2 and model._attn_anchors is None
        assert "anchors" not in model.attention_report()["attention_window"]
        same = model.set_attention_window(0, _N, anchors=(0, 0))(**inp).float().clone()
        assert not A.anchor_calls() and len(A.WINDOW_CALLS) == 4 and torch.equal(same, narrow)
        A.WINDOW_CALLS.clear()
        anchored = model.set_attention_window(0, _N, anchors=(1, 1))(**inp).float().clone()
    want = tuple(map(tuple, mmdit.attention_window_table(_LT, _T * _N, _N, 0, anchor_head=1, anchor_tail=1).tolist()))
    calls = A.anchor_calls()
    assert not A.WINDOW_CALLS and len(calls) == 2, calls
    assert all(c[0] == "bf16" and c[1:5] == (640, 640, 192, 128) and c[6] == want for c in calls), calls
    rep = model.attention_report()["attention_window"]
    assert rep["anchors"] == (1, 1) and rep["visited_tile_fraction"] == pytest.approx((5 * 3 + sum(r[1] for r in want)) / 30)
    e_narrow, e_anch = rel_l2(narrow, off), rel_l2(anchored, off)
    print(f"bf16 model on the CPU table: W = 0 vs off {e_narrow:.3e}; W = 0 with anchors (1, 1) vs off {e_anch:.3e}")
    assert torch.isfinite(anchored).all() and not torch.equal(anchored, narrow)
    # no body: refused when the forward sees the geometry; the environment variable; a table without the entry
    with pytest.raises(ValueError), torch.inference_mode():
        model.set_attention_window(0, _N, anchors=(3, 3))(**inp)
    with pytest.raises(ValueError):
        model.set_attention_window(0, _N, anchors=(-1, 0))
    assert model.set_attention_window(None)._attn_anchors is None


def test_environment_and_older_tables(anchor_ops, monkeypatch):
    mmdit = anchor_ops
    cfg, model = _model(mmdit)
    monkeypatch.setenv("OSK_ATTN_WINDOW_ANCHORS", "1,0")
    assert model.set_attention_window(1, _N)._attn_anchors == (1, 0)
    assert model.set_attention_window(1, _N, anchors=None)._attn_anchors is None
    monkeypatch.setenv("OSK_ATTN_WINDOW_ANCHORS", "0,0")
    assert model.set_attention_window(1, _N)._attn_anchors is None
    monkeypatch.setenv("OSK_ATTN_WINDOW_ANCHORS", "nonsense")
    with pytest.raises(ValueError):
        model.set_attention_window(1, _N)
    monkeypatch.delenv("OSK_ATTN_WINDOW_ANCHORS")
    from tests import cpu_ops_window as W

    mmdit.set_ops_for_testing(W)                                         # a table from before the entry: anchors refused, the rest works
    with pytest.raises(ValueError):
        model.set_attention_window(1, _N, anchors=(1, 0))
    assert model.set_attention_window(1, _N)._attn_window == (1, _N)


@pytest.mark.parametrize("hd", [72, 128])
def test_fp8_model_calls_the_anchor_entry_in_its_mode(anchor_ops, hd):
    mmdit = anchor_ops
    mode = MODELS[hd][1]
    model = build(mmdit, hd)
    x = model_case(hd)[2]
    with torch.inference_mode():
        narrow = model.set_attention_window(0, _N)(**x).float().clone()
        assert len(A.WINDOW_FP8_CALLS) == 2 and not A.anchor_calls()
        anchored = model.set_attention_window(0, _N, anchors=(1, 0))(**x).float().clone()
    want = tuple(map(tuple, mmdit.attention_window_table(_LT, _T * _N, _N, 0, anchor_head=1).tolist()))
    calls = A.anchor_calls()
    assert len(A.WINDOW_FP8_CALLS) == 2 and len(calls) == 2 and all(c[0] == mode and c[1:5] == (640, 640, 192, 0) and c[6] == want for c in calls), calls
    assert model.attention_report()["attention_window"]["mode"] == mode
    print(f"hd {hd} {mode}: W = 0 anchors (1, 0) vs none on the CPU table relL2 {rel_l2(anchored, narrow):.3e}")
    assert torch.isfinite(anchored).all() and not torch.equal(anchored, narrow)


# ----------------------------------------------------------------------------- the sampler
def test_cond_anchor_frames(hip_lib):
    from open_sora_amd.sampling import cond_anchor_frames

    def masks(on, B=2, T=5):
        m = torch.zeros(B, 1, T, 4, 6)
        for f in on:
            m[:, :, f] = 1
        return m

    assert cond_anchor_frames(masks([0])) == (1, 0)                      # i2v_head
    assert cond_anchor_frames(masks([4])) == (0, 1)                      # i2v_tail
    assert cond_anchor_frames(masks([0, 4])) == (1, 1)                   # i2v_loop
    assert cond_anchor_frames(masks([])) == (0, 0)                       # text-to-video
    assert cond_anchor_frames(masks([0, 1, 2])) == (3, 0) and cond_anchor_frames(masks([0, 3, 4])) == (1, 2)
    assert cond_anchor_frames(masks([0, 2])) == (1, 0)                   # an interior frame is no anchor
    assert cond_anchor_frames(masks(range(5))) == (5, 0)
    m = masks([0, 4])
    m[1, :, 4] = 0                                                       # every sample has to carry the frame
    assert cond_anchor_frames(m) == (1, 0)
    m = masks([0])
    m[0, 0, 0, 1, 1] = 0                                                 # and every position of it
    assert cond_anchor_frames(m) == (0, 0)


def test_denoise_takes_anchors_and_restores_the_setting(anchor_ops):
    from open_sora_amd import sampling

    cfg, model = _model(anchor_ops)
    n, T, Hh, Ww, Lt = 1, 4, 16, 24, 64                      # 96 tokens per latent frame at patch size 2
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
        with pytest.raises(ValueError):
            den.denoise(model, attn_window_anchors=(1, 0), **dict(args))
        plain = den.denoise(model, attn_window_frames=0, **dict(args))
        assert not A.anchor_calls() and len(A.WINDOW_CALLS) == 3 * 2
        cond = den.denoise(model, attn_window_frames=0, attn_window_anchors="cond", **dict(args))
        calls = A.anchor_calls()
        assert len(calls) == 3 * 2 and all(c[3:5] == (192, 0) for c in calls) and model._attn_window is None and model._attn_anchors is None
        explicit = den.denoise(model, attn_window_frames=0, attn_window_anchors=(1, 0), cfg_prune=True, **dict(args))
        assert torch.isfinite(cond.float()).all() and not torch.equal(cond, plain) and torch.isfinite(explicit.float()).all()
        # text-to-video masks: "cond" gives no anchors, the calls from before
        A.ANCHOR_CALLS.clear()
        den.denoise(model, attn_window_frames=0, attn_window_anchors="cond", **dict(args, masks=torch.zeros_like(masks)))
        assert not A.anchor_calls()
        # the model's own setting, anchors included, comes back
        model.set_attention_window(2, 96, anchors=(0, 1))
        den.denoise(model, attn_window_frames=1, attn_window_anchors=(1, 1), **dict(args))
        assert model._attn_window == (2, 96) and model._attn_anchors == (0, 1)
        den.denoise(model, attn_window_frames=1, **dict(args))
        assert model._attn_window == (2, 96) and model._attn_anchors == (0, 1)


# ----------------------------------------------------------------------------- sequence parallelism, ranks as threads
def _run_sp(model, inp, P, mode):
    from open_sora_amd import seqpar

    def rank_fn(rank, world):
        m = copy.copy(model)
        m.forward = m.forward_ckpt
        object.__setattr__(m, "_osk_ws_cache", {})
        sp = seqpar.enable(m, mode=mode, transport=LocalTransport(world, rank, "cpu"))
        with torch.inference_mode():
            out = m(**inp).float().clone()
        return out, threading.get_ident(), sp

    A.ANCHOR_CALLS.clear()
    res = run_ranks(P, rank_fn, "cpu")
    return [(out, list(A.ANCHOR_CALLS.get(ident, [])), sp) for out, ident, sp in res]


@pytest.mark.parametrize("mode", ["allgather", "ulysses"])
def test_every_rank_calls_the_anchor_entry_with_the_table_of_its_rows(anchor_ops, mode):
    """256 text + 6 frames x 128 tokens over P = 2: Lc = 512, a rank's blocks are the single-device blocks, so the sharded anchored
    forward computes the single-device anchored forward.  Bound: the 2^-7 the suite holds a sharded forward to."""
    mmdit = anchor_ops
    cfg, model = _sp_model(mmdit)
    inp = torch_inputs(cfg, 1, 6, 8, 16, 256, dtype=BF)
    model.set_attention_window(1, 128, anchors=(1, 1))
    with torch.inference_mode():
        single = model(**inp).float().clone()
        plain = model.set_attention_window(1, 128)(**inp).float().clone()
    model.set_attention_window(1, 128, anchors=(1, 1))
    res = _run_sp(model, inp, 2, mode)
    bounds = mmdit.attention_window_bounds(256, 768, 128, 1, 1)
    assert bounds == (384, 128)
    full = tuple(map(tuple, mmdit.attention_window_table(256, 768, 128, 1, anchor_head=1, anchor_tail=1).tolist()))
    for rank, (out, calls, sp) in enumerate(res):
        assert sp.geom == (512, 512) and torch.equal(out, res[0][0])
        assert all(c[0] == "bf16" and c[1:5] == (512, 1024) + bounds for c in calls), calls
        if mode == "allgather":
            assert len(calls) == 2 and all(c[6] == full[2 * rank: 2 * rank + 2] for c in calls), calls
            want = tuple(map(tuple, mmdit.attention_window_table(256, 768, 128, 1, row0=512 * rank, n_rows=512, anchor_head=1, anchor_tail=1).tolist()))
            assert calls[0][6] == want
        else:
            assert len(calls) == 4 and [c[6] for c in calls] == [full[0:2], full[2:4]] * 2
    e, sep = rel_l2(res[0][0], single), rel_l2(plain, single)
    print(f"P = 2 {mode}: relL2 sharded vs single-device anchored {e:.3e}; the anchors move the windowed forward by {sep:.3e}")
    assert e <= min(2.0 ** -7, sep / 2), (e, sep)


def test_ragged_split_with_anchors(anchor_ops):
    """64 + 6 x 96 = 640 rows over P = 3 (214, 214, 212), all-gather: every rank's table is that of its own rows"""
    mmdit = anchor_ops
    cfg, model = _sp_model(mmdit)
    inp = torch_inputs(cfg, 1, _T, 8, 12, _LT, dtype=BF)
    model.set_attention_window(0, _N, anchors=(1, 1))
    res = _run_sp(model, inp, 3, "allgather")
    for rank, (out, calls, sp) in enumerate(res):
        rows = 214 if rank < 2 else 212
        want = tuple(map(tuple, mmdit.attention_window_table(_LT, _T * _N, _N, 0, row0=214 * rank, n_rows=rows, anchor_head=1, anchor_tail=1).tolist()))
        assert len(calls) == 2 and all(c[1:5] == (rows, 640, 192, 128) and c[6] == want for c in calls), (rank, calls)
        assert torch.isfinite(out).all() and torch.equal(out, res[0][0])
