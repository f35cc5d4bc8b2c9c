"""GPU: the sampler's attention broadcast.  (1) osk_attn_cache_copy_bf16 (csrc/attn_cache.hip) bit for bit against the torch indexing
it states, strided on either side, with and without a row map, guard bands untouched; (2) MMDiTModel.forward_ckpt(attn_cache=...) on
a tiny denoiser (depth 2 + 2, 64 text + 2 frames of image tokens, B 3): a store step is the plain step, a reuse step on the same
inputs is the store step, a reuse step on other inputs is the block sequence driven by hand from the existing ops with the stored
attention tensor substituted -- in bf16, fp8 (pv8), qk8 (head_dim 128) and with the frame window; (3) I2VDenoiser.denoise(
attn_broadcast=...) against the loop driven by hand from forward_ckpt, also under cfg_prune and hip_graph.  All comparisons are of
bits; the one figure (how far broadcasting moves the result) is printed, not gated (pytest -s)."""
import functools

import pytest
import torch

from oracle import configs, sampling_oracle as S
from tests.test_attn_broadcast_host import _hand_loop
from tests.test_gpu_mmdit import _build
from tests.test_gpu_row_kernels import assert_guards, assert_rest_untouched, bits, guarded, sentinel
from tests.util import rel_l2, torch_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
ALL = slice(None)

# (B, L, C): the two shapes of the issue; L * C / 8 no multiple of the 256-lane workgroup with C = 8; more chunks than one pass of the
# 2048 x 256 grid (3 * 1500 * 144 = 648000 > 524288)
COPY_SHAPES = {"b3_l200_c128": (3, 200, 128), "b2_l65_c144": (2, 65, 144), "c8_odd_l": (3, 33, 8), "grid_stride": (3, 1500, 1152)}
ROW_MAPS = {"identity_map": (0, 1, 2), "swap": (2, 0), "one": (1,), "null": None}


@functools.lru_cache(maxsize=None)
def _values(name: str) -> torch.Tensor:
    """CPU bf16 [3, L, C] with every element distinct enough to tell rows apart; computed once, left unchanged"""
    B, L, C = COPY_SHAPES[name]
    g = torch.Generator().manual_seed(97 + len(name))
    return torch.randn(3, L, C, generator=g).to(BF)


# every shape with every map that names no more batch items than the shape has
COPY_CASES = [(s, m) for s in COPY_SHAPES for m in ROW_MAPS if ROW_MAPS[m] is None or len(ROW_MAPS[m]) <= COPY_SHAPES[s][0]]


@pytest.mark.parametrize("name,map_name", COPY_CASES, ids=[f"{s}-{m}" for s, m in COPY_CASES])
def test_cache_copy_is_the_indexing_it_states(hip_lib, name, map_name):
    Bs, L, C = COPY_SHAPES[name]
    rows = ROW_MAPS[map_name]
    B = Bs if rows is None else len(rows)
    idx = list(range(B)) if rows is None else list(rows)
    cache_rows = 3
    row_map = None if rows is None else torch.tensor(rows, dtype=torch.int32, device=DEV)
    vals = _values(name)
    D, R = C, 4 * C                                        # the workspace's single-block row: [q | k | v | mlp], row stride 3 D + R
    # --- store: the v columns of a y-layout buffer -> a contiguous slot between guard bands
    y = torch.zeros(B, L, 3 * D + R, dtype=BF)
    y[:, :, 2 * D: 3 * D] = vals[:B]
    y_d = y.to(DEV)
    n = cache_rows * L * C
    flat, slot = guarded(n, BF)
    slot = slot.view(cache_rows, L, C)
    before = flat.clone()
    hip_lib.attn_cache_copy(y_d[:, :, 2 * D: 3 * D], slot, row_map, True)
    torch.cuda.synchronize()
    assert_guards(flat, n)
    want = before[64: 64 + n].view(cache_rows, L, C).clone()
    want[idx] = y_d[:, :, 2 * D: 3 * D]
    assert torch.equal(bits(slot), bits(want)), "store: dst[row_map[b]] != src[b], or a row outside the map was written"
    assert torch.equal(bits(y_d.cpu()), bits(y)), "store wrote its source"
    # --- load: a contiguous slot -> the v columns of a sentinel-filled y-layout buffer (everything around them stays)
    slot_d = vals.to(DEV)
    out = sentinel((B, L, 3 * D + R), BF)
    out_before = out.clone()
    hip_lib.attn_cache_copy(slot_d, out[:, :, 2 * D: 3 * D], row_map, False)
    torch.cuda.synchronize()
    assert torch.equal(bits(out[:, :, 2 * D: 3 * D].cpu()), bits(vals[idx])), "load: dst[b] != src[row_map[b]]"
    assert_rest_untouched(out, out_before, (ALL, ALL, slice(2 * D, 3 * D)))
    assert torch.equal(bits(slot_d.cpu()), bits(vals)), "load wrote its source"
    # --- both sides strided: the double block's y ([q | k | v], row stride 3 D) into a slot that is a column slice of a wider buffer
    wide_flat, wide = guarded(cache_rows * L * (C + 16), BF)
    wide = wide.view(cache_rows, L, C + 16)
    wide_before = wide.clone()
    y3 = torch.zeros(B, L, 3 * D, dtype=BF, device=DEV)
    y3[:, :, 2 * D:] = vals[:B].to(DEV)
    hip_lib.attn_cache_copy(y3[:, :, 2 * D:], wide[:, :, 8: 8 + C], row_map, True)
    torch.cuda.synchronize()
    assert_guards(wide_flat, cache_rows * L * (C + 16))
    assert torch.equal(bits(wide[idx][:, :, 8: 8 + C].cpu()), bits(vals[:B]))
    assert_rest_untouched(wide, wide_before, (idx, ALL, slice(8, 8 + C)))


def test_a_map_entry_outside_the_slot_is_skipped_and_bad_arguments_launch_nothing(hip_lib):
    L, C = 16, 32
    src = torch.randn(3, L, C, device=DEV).to(BF)
    flat, slot = guarded(2 * L * C, BF)
    slot = slot.view(2, L, C)
    before = flat.clone()
    hip_lib.attn_cache_copy(src, slot, torch.tensor([1, 2, -1], dtype=torch.int32, device=DEV), True)      # rows 2 and -1: outside [0, 2)
    torch.cuda.synchronize()
    assert_guards(flat, 2 * L * C)
    assert torch.equal(bits(slot[1]), bits(src[0])) and torch.equal(bits(slot[0]), bits(before[64: 64 + L * C].view(L, C)))
    now = flat.clone()
    for bad in (lambda: hip_lib.attn_cache_copy(src, slot, None, True),                                          # 3 items, 2 rows, no map
                lambda: hip_lib.attn_cache_copy(src[:, :, 4:28], slot[:, :, :24], None, True),                   # 8-byte aligned only
                lambda: hip_lib.attn_cache_copy(src[:2, :8], slot, None, True),                                  # L differs
                lambda: hip_lib.attn_cache_copy(src[:2], slot, torch.tensor([0, 1], device=DEV), True),          # int64 map
                lambda: hip_lib.attn_cache_copy(src[:2], slot, torch.tensor([0, 1], dtype=torch.int32), True),   # map on the host
                lambda: hip_lib.attn_cache_copy(slot, slot, None, True),                                         # overlap
                lambda: hip_lib.attn_cache_copy(src[:2].float(), slot, None, True)):
        with pytest.raises(ValueError, match="osk_attn_cache_copy_bf16"):
            bad()
    torch.cuda.synchronize()
    assert torch.equal(bits(flat), bits(now))


# ----------------------------------------------------------------------------- the model
B_, T_, H_, W_, LT_ = 3, 2, 6, 6, 64                        # 64 text + 2 frames x 36 image tokens = 136 rows; B L = 408 (fp8 GEMM: M >= 256)
FRAME = H_ * W_
MODES = ["bf16", "fp8", "qk8", "window", "window_fp8"]


def _tiny(mode: str):
    name = "hd128_liger_split" if mode == "qk8" else "hd72_eager_split"
    cfg = dict(configs.GOLDEN[name][0], depth=2, depth_single_blocks=2)
    model = _build(cfg)
    if mode in ("fp8", "window_fp8"):
        model.enable_fp8()
    if mode == "qk8":
        model.enable_fp8(qk8=True)
    if mode in ("window", "window_fp8"):
        model.set_attention_window(1, FRAME)
    return cfg, model


def _shift(inp, s):
    return dict(inp, img=(inp["img"].float() * (1.0 + s)).to(BF), timesteps=(inp["timesteps"].float() * (1.0 - s)).to(BF))


def _hand_reuse(model, inp, stored):
    """a reuse step as the block sequence it states, driven by hand from the existing ops: the forward's head, then per double
    block the two attention projections on the stored tensor, second LN + modulate and the MLP; per single block LN + modulate, the
    MLP-up columns of linear1, the stored tensor into the v columns (torch's copy), linear2; then the forward's tail"""
    from open_sora_amd import mmdit as M

    D, H = model.hidden_size, model.num_heads
    R = int(D * model.config.mlp_ratio)
    st = model._forward_head(None, None, inp["img"], inp["img_ids"], inp["txt"], inp["txt_ids"], inp["timesteps"], inp["y_vec"],
                             inp.get("cond"), inp.get("guidance"))
    ws, mod, p = st.ws, st.mod, st.plan
    Lt = ws.L_txt
    x_txt, x_img, xm_txt, xm_img = ws.x[:, :Lt], ws.x[:, Lt:], ws.xm[:, :Lt], ws.xm[:, Lt:]
    blocks = iter(stored)
    for plan, (ci, ct) in zip(p["double"], p["col_double"]):
        v = next(blocks)
        (_, _, i_g1, i_sh2, i_sc2, i_g2), mbs = M._mod_views(mod, ci, 6, D)
        (_, _, t_g1, t_sh2, t_sc2, t_g2), _ = M._mod_views(mod, ct, 6, D)
        M._linear_pair(dict(a=v[:, Lt:], w=plan.img.proj_w, bias=plan.img.proj_b, out=x_img, res=x_img, gate=i_g1, gate_batch_stride=mbs),
                       dict(a=v[:, :Lt], w=plan.txt.proj_w, bias=plan.txt.proj_b, out=x_txt, res=x_txt, gate=t_g1, gate_batch_stride=mbs))
        (iw0, ib0, iw2, ib2), (tw0, tb0, tw2, tb2) = plan.img_mlp, plan.txt_mlp
        a_img = M._ln_modulate_for(iw0, x_img, i_sh2, i_sc2, xm_img, mbs)
        a_txt = M._ln_modulate_for(tw0, x_txt, t_sh2, t_sc2, xm_txt, mbs)
        M._linear_pair(dict(a=a_img, w=iw0, bias=ib0, out=ws.h[:, Lt:]), dict(a=a_txt, w=tw0, bias=tb0, out=ws.h[:, :Lt]), gelu_from=0)
        M._linear_pair(dict(a=ws.h[:, Lt:], w=iw2, bias=ib2, out=x_img, res=x_img, gate=i_g2, gate_batch_stride=mbs),
                       dict(a=ws.h[:, :Lt], w=tw2, bias=tb2, out=x_txt, res=x_txt, gate=t_g2, gate_batch_stride=mbs))
    for plan, c in zip(p["single"], p["col_single"]):
        y = ws.y_single(D, R)
        (shift, scale, gate), mbs = M._mod_views(mod, c, 3, D)
        act = M._ln_modulate_for(plan.w1, ws.x, shift, scale, ws.xm, mbs)
        M._linear(act, plan.w1[3 * D:], None if plan.b1 is None else plan.b1[3 * D:], y[:, :, 3 * D:], gelu_from=0)
        y[:, :, 2 * D: 3 * D].copy_(next(blocks))
        M._linear(y[:, :, 2 * D:], plan.w2, plan.b2, ws.x, res=ws.x, gate=gate, gate_batch_stride=mbs)
    return model._forward_tail(st).clone()


@pytest.mark.parametrize("mode", MODES)
def test_store_is_plain_and_reuse_is_the_stored_attention(hip_lib, mode):
    from open_sora_amd import mmdit

    if mode in ("window_fp8",) and not mmdit._window_fp8_ok():
        pytest.skip("no fp8 window entry in this library")
    cfg, model = _tiny(mode)
    a = torch_inputs(cfg, B_, T_, H_, W_, LT_, dtype=BF, device=DEV)
    b = _shift(a, 0.125)
    rows = (0, 1, 2)
    with torch.inference_mode():
        plain = model(**a).clone()
        ac = model.attention_broadcast_begin(B_, LT_, T_ * FRAME, DEV)
        ptr = ac.slots.data_ptr()
        store = model(**a, attn_cache=(ac, "store", rows)).clone()
        again = model(**a, attn_cache=(ac, "reuse", rows)).clone()
        stored = ac.slots.clone()
        other = model(**b, attn_cache=(ac, "reuse", rows)).clone()
        torch.cuda.synchronize()
        assert torch.equal(bits(ac.slots), bits(stored)), "a reuse step wrote the cache"
        hand = _hand_reuse(model, b, stored)
        plain_b = model(**b).clone()
        torch.cuda.synchronize()
    assert torch.isfinite(plain.float()).all() and float(stored.float().abs().sum()) > 0.0
    assert torch.equal(bits(store), bits(plain)), "(i) a store step is not the plain step"
    assert torch.equal(bits(again), bits(store)), "(ii) a reuse step on the same inputs is not the store step"
    assert torch.equal(bits(other), bits(hand)), "(iii) a reuse step is not the hand-driven block sequence on the stored tensor"
    assert not torch.equal(bits(other), bits(plain_b))
    assert model.attention_broadcast_begin(B_, LT_, T_ * FRAME, DEV).slots.data_ptr() == ptr      # allocated once, never moves
    print(f"[{mode}] reuse on shifted inputs vs their own plain step: relL2 {rel_l2(other, plain_b):.3e} (recorded, not gated)")


# ----------------------------------------------------------------------------- the sampler
STEPS = 8
_SHIPPED = dict(guidance=7.5, guidance_img=3.0, text_osci=True, image_osci=True, scale_temporal_osci=True)


@functools.lru_cache(maxsize=None)
def _case():
    """image-to-video inputs as tests/test_gpu_step_cache.py makes them (CPU, bf16-representable f32), 8 steps; left unchanged"""
    from open_sora_amd import sampling

    cfg = dict(configs.GOLDEN["hd72_eager_split"][0], depth=2, depth_single_blocks=2)
    n, T, Hh, Ww, Lt = 1, 2, 12, 12, 64
    g = torch.Generator().manual_seed(31)
    z = torch.randn(n, 16, T, Hh, Ww, generator=g).bfloat16().float()
    masks = torch.zeros(n, 1, T, Hh, Ww)
    masks[:, :, 0] = 1
    masked_ref = (torch.randn(n, 16, T, Hh, Ww, generator=g) * masks).bfloat16().float()
    txt = (torch.randn(3 * n, Lt, cfg["context_in_dim"], generator=g) * 0.2).bfloat16().float()
    y_vec = torch.randn(3 * n, cfg["vec_in_dim"], generator=g).bfloat16().float()
    img_ids, txt_ids = S.grid_ids(3 * n, T, Hh // 2, Ww // 2, Lt, torch.float32)
    ts = sampling.get_schedule(STEPS, (Hh // 2) * (Ww // 2), T)
    tensors = dict(img=S.pack(z).repeat(3, 1, 1), masks=masks, masked_ref=masked_ref, img_ids=img_ids, txt=txt, txt_ids=txt_ids, y_vec=y_vec)
    return cfg, tensors, dict(timesteps=ts, **_SHIPPED)


def _to(tensors, dev):
    return {k: v.to(dev, BF) for k, v in tensors.items()}


@functools.lru_cache(maxsize=None)
def _sampler_model():
    return _build(_case()[0])


WANT = ["plain", "plain", "store", "reuse", "store", "reuse", "plain", "plain"]


def test_loop_is_the_loop_driven_by_hand_and_moves_the_result(hip_lib, monkeypatch):
    from open_sora_amd import sampling

    monkeypatch.delenv("OSK_ATTN_BROADCAST", raising=False)
    cfg, tensors, kw = _case()
    ts = kw["timesteps"]
    rng = (ts[6], ts[2])                                  # covers steps 2 .. 6
    assert sampling.attn_broadcast_plan(ts, 2, rng) == WANT
    model = _sampler_model()
    with torch.inference_mode():
        den = sampling.I2VDenoiser()
        out = den.denoise(model, attn_broadcast=2, attn_broadcast_range=rng, **_to(tensors, DEV), **kw)
        hand = _hand_loop(model, tensors, kw, WANT, dev=DEV, ops=hip_lib)
        plain = sampling.I2VDenoiser().denoise(model, **_to(tensors, DEV), **kw)
        torch.cuda.synchronize()
    assert den.last_attn_broadcast == WANT and torch.isfinite(out.float()).all()
    assert torch.equal(bits(out), bits(hand))
    assert not torch.equal(bits(out), bits(plain)), "attention broadcast did not change the result: is it on?"
    print(f"attn_broadcast=2 over steps 2..6 of {STEPS} vs the unbroadcast loop: relL2 {rel_l2(out, plain):.3e} (recorded, not gated)")


def test_loop_with_cfg_prune_falls_back_to_a_computed_step(hip_lib, monkeypatch):
    from open_sora_amd import sampling

    counts = [3, 3, 1, 3, 1, 1, 3, 3]                     # step 3 reuses rows 1 and 2 that step 2 (one branch) did not store
    monkeypatch.setattr(sampling, "cfg_branch_counts", lambda *a, **k: list(counts))
    cfg, tensors, kw = _case()
    ts = kw["timesteps"]
    rng = (ts[6], ts[2])
    model = _sampler_model()
    want = ["plain", "plain", "store", "store", "store", "reuse", "plain", "plain"]
    assert sampling.attn_broadcast_effective(WANT, counts) == want
    with torch.inference_mode():
        den = sampling.I2VDenoiser()
        out = den.denoise(model, attn_broadcast=2, attn_broadcast_range=rng, cfg_prune=True, **_to(tensors, DEV), **kw)
        hand = _hand_loop(model, tensors, kw, want, counts, dev=DEV, ops=hip_lib)
        torch.cuda.synchronize()
    assert den.last_attn_broadcast == want and den.last_branch_counts == counts
    assert torch.equal(bits(out), bits(hand))


@pytest.mark.parametrize("pruned", [False, True], ids=["triple", "cfg_prune"])
def test_graph_replay_equals_eager(hip_lib, monkeypatch, pruned):
    from open_sora_amd import sampling

    counts = [3, 3, 1, 3, 1, 1, 3, 3]
    if pruned:
        monkeypatch.setattr(sampling, "cfg_branch_counts", lambda *a, **k: list(counts))
    cfg, tensors, kw = _case()
    ts = kw["timesteps"]
    rng = (ts[6], ts[1])                                  # steps 1 .. 6: store reuse store reuse store reuse -- every graph replays
    model = _sampler_model()
    with torch.inference_mode():
        eager = sampling.I2VDenoiser().denoise(model, attn_broadcast=2, attn_broadcast_range=rng, cfg_prune=pruned, **_to(tensors, DEV), **kw)
        den = sampling.I2VDenoiser()
        graph = den.denoise(model, attn_broadcast=2, attn_broadcast_range=rng, cfg_prune=pruned, hip_graph=True, **_to(tensors, DEV), **kw)
        torch.cuda.synchronize()
    assert "store" in den.last_attn_broadcast and "reuse" in den.last_attn_broadcast
    assert torch.isfinite(eager.float()).all() and torch.equal(bits(eager), bits(graph))
