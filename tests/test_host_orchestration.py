"""CPU: the host-side orchestration of open_sora_amd.mmdit (joint [txt;img] buffers, in-place v-slot reuse,
batched adaLN columns, K padding of the embedders, processor plug-ins) driven through a CPU emulation of the
kernels' semantics (tests/cpu_ops.py) and compared with the goldens made by the REAL reference.  This is host
logic only — the kernels themselves are checked on the GPU by tests/test_gpu_*.py."""
import os

import numpy as np
import pytest
import torch

from oracle import configs, mmdit_oracle as O
from tests import cpu_ops
from tests.util import assert_parity, torch_inputs, torch_params

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BF = torch.bfloat16


@pytest.fixture()
def cpu_mmdit(hip_lib):
    from open_sora_amd import mmdit

    mmdit.set_ops_for_testing(cpu_ops)
    yield mmdit
    mmdit.set_ops_for_testing(hip_lib)


def _build(mmdit, cfg):
    model = mmdit.Flux(device_map="cpu", torch_dtype=BF, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=BF), strict=True)
    return model


@pytest.mark.parametrize("name", list(configs.GOLDEN))
def test_engine_orchestration_vs_golden(cpu_mmdit, name):
    cfg, B, T, h, w, L_txt = configs.GOLDEN[name]
    truth = torch.from_numpy(np.load(os.path.join(GOLDEN_DIR, f"mmdit_{name}.npz"))["out"])
    model = _build(cpu_mmdit, cfg)
    inp = torch_inputs(cfg, B, T, h, w, L_txt, dtype=BF)
    with torch.inference_mode():
        out = model(**inp)
        ref_bf16 = O.forward(torch_params(cfg, dtype=BF), cfg, **inp)
    assert_parity(out, truth, ref_bf16, f"host orchestration [{name}]")


def test_processors_on_reference_style_pe(cpu_mmdit):
    cfg, B, T, h, w, L_txt = configs.GOLDEN["hd64_eager_fused"]
    model = _build(cpu_mmdit, cfg)
    sd32 = torch_params(cfg)
    inp32 = torch_inputs(cfg, B, T, h, w, L_txt)
    with torch.inference_mode():
        img, txt, vec, ang = O.prepare_block_inputs(sd32, cfg, **inp32)
        c, s = torch.cos(ang), torch.sin(ang)
        pe = torch.stack([c, -s, s, c], dim=-1).reshape(*ang.shape, 2, 2).float().unsqueeze(1)
        t_img, t_txt = O.double_block(sd32, cfg, 0, img, txt, vec, ang, "interleaved")
        sdb = {k: v.bfloat16() for k, v in sd32.items()}
        r_img, r_txt = O.double_block(sdb, cfg, 0, img.bfloat16(), txt.bfloat16(), vec.bfloat16(), ang, "interleaved")
        img_b, txt_b = img.bfloat16(), txt.bfloat16()
        keep = (img_b.clone(), txt_b.clone())
        o_img, o_txt = model.double_blocks[0](img_b, txt_b, vec.bfloat16(), pe)
        # bf16 callers: the kernels read the caller's tensors in place and write fresh outputs -- the inputs must come back untouched
        assert torch.equal(img_b, keep[0]) and torch.equal(txt_b, keep[1])
        assert o_img.data_ptr() != img_b.data_ptr() and o_img.is_contiguous() and o_txt.is_contiguous()
        assert_parity(o_img, t_img, r_img, "double processor img")
        assert_parity(o_txt, t_txt, r_txt, "double processor txt")
        x = torch.cat((t_txt, t_img), 1)
        t_x = O.single_block(sd32, cfg, 0, x, vec, ang, "interleaved")
        r_x = O.single_block(sdb, cfg, 0, x.bfloat16(), vec.bfloat16(), ang, "interleaved")
        x_b = x.bfloat16()
        keep_x = x_b.clone()
        o_x = model.single_blocks[0](x_b, vec.bfloat16(), pe)
        assert torch.equal(x_b, keep_x) and o_x.data_ptr() != x_b.data_ptr()
        # a caller in another dtype is staged through the workspace and gets its dtype back
        o_x32 = model.single_blocks[0](x_b.float(), vec.bfloat16().float(), pe)
        assert o_x32.dtype == torch.float32 and torch.equal(o_x32.bfloat16(), o_x)
        assert_parity(o_x, t_x, r_x, "single processor")


def test_processors_take_strided_caller_tensors(cpu_mmdit):
    """a NON-contiguous bf16 caller tensor -- the img half of a joint [txt; img] buffer, a column slice of a
    wider tensor -- must not be handed to the GEMM as its residual (the ABI carries one set of strides for C and res): it is
    staged through the workspace and gives the contiguous call's result bit for bit."""
    cfg, B, T, h, w, L_txt = configs.GOLDEN["hd64_eager_fused"]
    model = _build(cpu_mmdit, cfg)
    sd32 = torch_params(cfg)
    with torch.inference_mode():
        img, txt, vec, ang = O.prepare_block_inputs(sd32, cfg, **torch_inputs(cfg, B, T, h, w, L_txt))
        c, s = torch.cos(ang), torch.sin(ang)
        pe = torch.stack([c, -s, s, c], dim=-1).reshape(*ang.shape, 2, 2).float().unsqueeze(1)
        img_b, txt_b, vec_b = img.bfloat16(), txt.bfloat16(), vec.bfloat16()
        o_img, o_txt = model.double_blocks[0](img_b, txt_b, vec_b, pe)
        joint = torch.cat((txt_b, img_b), 1)                                    # [B, Lt + Li, D]
        Lt = txt_b.shape[1]
        assert not joint[:, Lt:].is_contiguous() or B == 1
        wide = torch.zeros(B, img_b.shape[1], img_b.shape[2] + 64, dtype=BF)
        wide[:, :, :img_b.shape[2]] = img_b
        for i_view in (joint[:, Lt:], wide[:, :, :img_b.shape[2]]):
            s_img, s_txt = model.double_blocks[0](i_view, joint[:, :Lt], vec_b, pe)
            assert torch.equal(s_img, o_img) and torch.equal(s_txt, o_txt)
        x_b = torch.cat((o_txt, o_img), 1)
        o_x = model.single_blocks[0](x_b, vec_b, pe)
        wide_x = torch.zeros(B, x_b.shape[1], x_b.shape[2] + 64, dtype=BF)
        wide_x[:, :, :x_b.shape[2]] = x_b
        assert torch.equal(model.single_blocks[0](wide_x[:, :, :x_b.shape[2]], vec_b, pe), o_x)


def test_pe_memo_is_not_fooled_by_refilled_inference_tensors(cpu_mmdit):
    """a pe buffer created under inference_mode keeps no version counter and CAN be refilled in place there --
    the conversion memo must not serve the old cos / sin for it."""
    with torch.inference_mode():
        pe = torch.zeros(1, 1, 8, 4, 2, 2)
        pe[..., 0, 0] = 1.0
        c0, _, _ = cpu_mmdit._pe_to_cos_sin(pe, 8)
        assert float(c0.sum()) == 32.0
        pe[..., 0, 0] = 0.5
        c1, _, _ = cpu_mmdit._pe_to_cos_sin(pe, 8)
        assert float(c1.sum()) == 16.0
    pe2 = torch.zeros(1, 1, 8, 4, 2, 2)
    pe2[..., 0, 0] = 1.0
    a = cpu_mmdit._pe_to_cos_sin(pe2, 8)
    assert cpu_mmdit._pe_to_cos_sin(pe2, 8)[0] is a[0]          # ordinary tensors: memoised ...
    pe2[..., 0, 0] = 0.25
    assert float(cpu_mmdit._pe_to_cos_sin(pe2, 8)[0].sum()) == 8.0   # ... until written in place


def test_engine_takes_the_group_projection_path(cpu_mmdit):
    """round 6: the QKV projection of a block goes out as ONE osk_gemm_group_bf16 launch that writes V directly as V^T -- no
    osk_v_transpose_bf16 call is left in a forward where the geometry qualifies (hd 64 model: 2 D % 256 == 0), the golden still
    holds (test_engine_orchestration_vs_golden runs the same path), and a library that declines the group is handled by the
    single calls with the same result."""
    cfg, B, T, h, w, L_txt = configs.GOLDEN["hd64_eager_fused"]
    model = _build(cpu_mmdit, cfg)
    inp = torch_inputs(cfg, B, T, h, w, L_txt, dtype=BF)
    calls = {"group": 0, "vt": 0}
    real_group, real_vt = cpu_ops.gemm_group, cpu_ops.v_transpose

    def spy_group(tasks):
        calls["group"] += 1
        return real_group(tasks)

    def spy_vt(*a, **k):
        calls["vt"] += 1
        return real_vt(*a, **k)

    cpu_ops.gemm_group, cpu_ops.v_transpose = spy_group, spy_vt
    try:
        with torch.inference_mode():
            out = model(**inp)
            n_blocks = cfg["depth"] + cfg["depth_single_blocks"]
            if L_txt % 64 == 0:
                assert calls["group"] == n_blocks, calls
            # the emulation's own V^T task calls v_transpose once per task; the ENGINE must not call it for qualifying blocks
            cpu_ops.gemm_group = lambda tasks: False            # a library that declines every group
            model._osk_ws_cache.clear()
            calls["vt"] = 0
            out2 = model(**inp)
            assert calls["vt"] == n_blocks                      # the legacy path: one osk_v_transpose_bf16 per block
    finally:
        cpu_ops.gemm_group, cpu_ops.v_transpose = real_group, real_vt
    d = (out.float() - out2.float()).abs().max()
    assert d <= 2.0 ** -6 * out2.float().abs().max() + 1e-3, d


def test_blocks_with_a_large_weight_bound_take_the_bound_from_their_operands(cpu_mmdit):
    """round 6: QK-norm scale vectors whose weight-derived bound exceeds the FAST limit (hd max|w_q| max|w_k| > 56 in log2 units) no
    longer send the block to the general attention body wholesale: the engine measures the row norms of the q / k it is about to
    multiply (osk_rownorm2_max_bf16) and calls the auto-dispatched attention with them; same result as the plain call."""
    cfg, B, T, h, w, L_txt = configs.GOLDEN["hd64_eager_fused"]
    model = _build(cpu_mmdit, cfg)
    with torch.no_grad():
        for blk in list(model.double_blocks) + list(model.single_blocks):
            for nrm in ([blk.img_attn.norm, blk.txt_attn.norm] if hasattr(blk, "img_attn") else [blk.norm]):
                nrm.query_norm.scale.mul_(3.0)
                nrm.key_norm.scale.mul_(3.0)
    inp = torch_inputs(cfg, B, T, h, w, L_txt, dtype=BF)
    calls = {"auto": 0, "norm": 0}
    real_auto, real_norm = cpu_ops.attention_fwd_auto, cpu_ops.rownorm2_max

    def spy_auto(*a, **k):
        calls["auto"] += 1
        return real_auto(*a, **k)

    def spy_norm(*a, **k):
        calls["norm"] += 1
        return real_norm(*a, **k)

    cpu_ops.attention_fwd_auto, cpu_ops.rownorm2_max = spy_auto, spy_norm
    try:
        with torch.inference_mode():
            out = model(**inp)
            rep = model.attention_report()
            n_blocks = cfg["depth"] + cfg["depth_single_blocks"]
            assert rep["score_bound_min"] > 56.0 and rep["blocks_auto_dispatched"] == n_blocks
            assert calls["auto"] == n_blocks and calls["norm"] == 2 * n_blocks
            cpu_mmdit.AUTO_BOUND = False
            out2 = model(**inp)
            assert calls["auto"] == n_blocks
    finally:
        cpu_ops.attention_fwd_auto, cpu_ops.rownorm2_max = real_auto, real_norm
        cpu_mmdit.AUTO_BOUND = True
    assert torch.equal(out, out2)


def test_processors_install_on_reference_blocks(cpu_mmdit):
    """The plug-in point of the reference itself: block.set_processor(...) on the reference's own
    DoubleStreamBlock / SingleStreamBlock (only where the reference tree is available, see oracle/ref_loader.py)."""
    from oracle import ref_loader

    if not ref_loader.available():
        pytest.skip(f"needs the reference tree (its own module classes are patched): none at {ref_loader.REF_ROOT}")
    cfg, B, T, h, w, L_txt = configs.GOLDEN["hd64_liger_split"]
    M, layers, _ = ref_loader.mmdit()
    ref = M.Flux(device_map="cpu", torch_dtype=torch.float32, **cfg)
    ref.load_state_dict(torch_params(cfg), strict=True)
    inp = torch_inputs(cfg, B, T, h, w, L_txt)
    with torch.inference_mode():
        truth = ref(**inp)
        refb = ref.to(BF)
        inpb = torch_inputs(cfg, B, T, h, w, L_txt, dtype=BF)
        ref_bf16 = refb(**inpb)
        for blk in refb.double_blocks:
            blk.set_processor(cpu_mmdit.HipDoubleStreamBlockProcessor())
        for blk in refb.single_blocks:
            blk.set_processor(cpu_mmdit.HipSingleStreamBlockProcessor())
        out = refb(**inpb)
    assert_parity(out, truth, ref_bf16, "reference model with our processors installed")


def test_sampler_loop_matches_reference_formula(cpu_mmdit):
    """I2VDenoiser.denoise against a direct transcription of sampling.py:181-222 around a stub model."""
    from open_sora_amd import sampling

    torch.manual_seed(0)
    n, T, Hh, Ww = 1, 2, 4, 6
    z = torch.randn(n, 16, T, Hh, Ww).to(BF)
    img = sampling.pack(z).repeat(3, 1, 1)
    masks = torch.zeros(n, 1, T, Hh, Ww, dtype=BF)
    masks[:, :, 0] = 1
    masked_ref = (torch.randn(n, 16, T, Hh, Ww) * masks).to(BF)
    ts = sampling.get_schedule(4, (Hh // 2) * (Ww // 2), T)
    W = torch.randn(64 + 68, 64) * 0.02

    def model(img, cond, timesteps, guidance, **kw):
        return (torch.cat([img.float(), cond.float()], -1) @ W * (1 + timesteps.float()[:, None, None])).to(BF)

    out = sampling.I2VDenoiser().denoise(model, img=img, timesteps=ts, guidance=7.5, guidance_img=3.0, masks=masks,
                                         masked_ref=masked_ref, sigma_min=1e-5, text_osci=True, image_osci=True,
                                         scale_temporal_osci=True)
    # transcription of the reference loop in fp32
    x = img[:n].float()
    cond = sampling.pack(torch.cat((masks, masked_ref), 1)).float()
    cond3 = torch.cat([cond, cond, torch.zeros_like(cond)])
    for i, (tc, tp) in enumerate(zip(ts[:-1], ts[1:])):
        tv = torch.full((3 * n,), tc, dtype=BF)
        pred = model(x.to(BF).repeat(3, 1, 1), cond3.to(BF), tv, None).float()
        tg = sampling.get_oscillation_gs(7.5, i)
        ig = sampling.get_oscillation_gs(3.0, i)
        c, u, u2 = pred.chunk(3)
        if ig > 1.0:
            upper = torch.linspace(ig, 1.0, len(ts))[i]
            ramp = torch.linspace(1.0, float(upper), T)[None, None, :, None, None].repeat(n, 16, 1, Hh, Ww)
            ig = sampling.pack(ramp)
        x = (x + (tp - tc) * (u2 + ig * (u - u2) + tg * (c - u))).to(BF).float()
    assert (out.float() - x).abs().max().item() <= 2e-2 * max(1.0, x.abs().max().item())


def test_pack_unpack_roundtrip_and_schedule(cpu_mmdit):
    from open_sora_amd import sampling

    z = torch.arange(2 * 16 * 3 * 8 * 12, dtype=torch.float32).reshape(2, 16, 3, 8, 12)
    p = sampling.pack(z)
    assert p.shape == (2, 3 * 4 * 6, 64)
    assert torch.equal(sampling.unpack(p, 8 * 8, 12 * 8, 3), z)
    # channel order (c ph pw), token order (t h w)  — sampling.py:375-378
    assert p[0, 0, 0] == z[0, 0, 0, 0, 0] and p[0, 0, 1] == z[0, 0, 0, 0, 1] and p[0, 0, 2] == z[0, 0, 0, 1, 0]
    assert p[0, 1, 0] == z[0, 0, 0, 0, 2] and p[0, 0, 4] == z[0, 1, 0, 0, 0]
    ts = sampling.get_schedule(30, 1024, 16)
    assert len(ts) == 31 and ts[0] == 1.0 and ts[-1] == 0.0 and all(a > b for a, b in zip(ts[:-1], ts[1:]))
    alpha = (1 + 2 / 3840 * (1024 - 256)) * 4.0  # sampling.py:295-332
    t1 = 1 - 1 / 30
    assert abs(ts[1] - alpha * t1 / (1 + (alpha - 1) * t1)) < 1e-6


def test_model_built_and_loaded_inside_inference_mode(cpu_mmdit):
    """the reference's scripts/diffusion/inference.py builds and loads every model inside `@torch.inference_mode() main()`:
    the parameters are then inference tensors, which track no version counter (`p._version` raises).  The plan keys must
    not read it (the first forward crashed), and the result must equal the model built outside."""
    name = "hd64_eager_fused"
    cfg, B, T, h, w, L_txt = configs.GOLDEN[name]
    inp = torch_inputs(cfg, B, T, h, w, L_txt, dtype=BF)
    outside = _build(cpu_mmdit, cfg)
    with torch.inference_mode():
        inside = _build(cpu_mmdit, cfg)
        assert all(p.is_inference() for p in inside.parameters())
        a = inside(**inp)
        a2 = inside(**inp)                      # second call: cached plan, same key
        b = outside(**inp)
        blk = inside.double_blocks[0]
        o_img, o_txt = blk(torch.zeros(1, 8, cfg["hidden_size"], dtype=BF), torch.zeros(1, 4, cfg["hidden_size"], dtype=BF),
                           torch.zeros(1, cfg["hidden_size"], dtype=BF),
                           (torch.ones(1, 12, cfg["hidden_size"] // cfg["num_heads"]), torch.zeros(1, 12, cfg["hidden_size"] // cfg["num_heads"])))
    assert torch.equal(a, b) and torch.equal(a, a2)
    assert o_img.shape == (1, 8, cfg["hidden_size"]) and o_txt.shape == (1, 4, cfg["hidden_size"])


def test_plan_key_sees_in_place_writes_but_not_data_writes(cpu_mmdit):
    """what the staleness key detects (autograd-visible in-place writes, storage swaps) and what it documents it does not
    (writes through `.data`: invalidate_plan() is the contract there)"""
    cfg, B, T, h, w, L_txt = configs.GOLDEN["hd64_eager_fused"]
    model = _build(cpu_mmdit, cfg)
    inp = torch_inputs(cfg, B, T, h, w, L_txt, dtype=BF)
    with torch.inference_mode():
        base = model(**inp)
    bias = model.final_layer.linear.bias        # the plan holds an f32 COPY of it (bf16 weights are aliased, not copied)
    with torch.no_grad():
        bias.add_(1.0)
    with torch.inference_mode():
        shifted = model(**inp)
    assert not torch.equal(shifted, base)       # rebuilt
    bias.data.sub_(1.0)                          # invisible to the key ...
    with torch.inference_mode():
        stale = model(**inp)
    assert torch.equal(stale, shifted)
    model.invalidate_plan()                      # ... so this is the documented contract
    with torch.inference_mode():
        fresh = model(**inp)
    assert torch.allclose(fresh.float(), base.float(), atol=2e-2, rtol=2e-2) and not torch.equal(fresh, shifted)


def test_block_level_load_state_dict_under_inference_mode_drops_the_plan(cpu_mmdit):
    """parameters that are inference tensors have no version counter, so an in-place `load_state_dict` on ONE BLOCK (or
    on one of its Linear layers) inside torch.inference_mode() changes the values without changing the plan key.  The load hooks
    drop the cached plan; the next forward equals a freshly built model with the same weights."""
    cfg, B, T, h, w, L_txt = configs.GOLDEN["hd64_eager_fused"]
    inp = torch_inputs(cfg, B, T, h, w, L_txt, dtype=BF)
    with torch.inference_mode():
        model = _build(cpu_mmdit, cfg)
        base = model(**inp)
        blk = model.double_blocks[0]
        sd = {k: (v * 1.5).to(v.dtype) for k, v in blk.state_dict().items()}
        blk.load_state_dict(sd)                                   # block level: the model's own override never runs
        assert "_osk_plan" not in blk.__dict__
        changed = model(**inp)
        lin = model.single_blocks[0].linear2
        lin.load_state_dict({k: (v * 0.5).to(v.dtype) for k, v in lin.state_dict().items()})   # a leaf of a single block
        assert "_osk_plan" not in model.single_blocks[0].__dict__
        changed2 = model(**inp)
        fresh = _build(cpu_mmdit, cfg)
        fresh.load_state_dict(model.state_dict())
        want = fresh(**inp)
    assert not torch.equal(changed, base) and not torch.equal(changed2, changed)
    assert torch.equal(changed2, want)


def test_workspace_cache_is_lru_and_caches_do_not_travel(cpu_mmdit):
    import copy

    cfg, B, T, h, w, L_txt = configs.GOLDEN["hd64_eager_fused"]
    model = _build(cpu_mmdit, cfg)
    with torch.inference_mode():
        for i, lt in enumerate((8, 16, 24, 32, 40)):              # five geometries: the oldest is evicted, not the whole cache
            model(**torch_inputs(cfg, B, T, h, w, lt, dtype=BF))
            if i == 3:
                keys4 = list(model._osk_ws_cache)
        keys5 = list(model._osk_ws_cache)
        assert len(keys5) == 4 and keys5[:3] == keys4[1:]
        model(**torch_inputs(cfg, B, T, h, w, 16, dtype=BF))      # a hit moves the entry to the young end
        assert list(model._osk_ws_cache)[-1] == keys5[0]
    clone = copy.deepcopy(model)
    assert "_osk_ws_cache" not in clone.__dict__ and clone._plan is None
    assert all("_osk_plan" not in b.__dict__ for b in clone.double_blocks)
    import pickle

    blob = pickle.dumps(model.double_blocks[0])     # the load_state_dict watchers are module-level functions: modules still pickle
    assert len(blob) < 3 * sum(p.numel() * p.element_size() for p in model.double_blocks[0].parameters())
    with torch.inference_mode():
        inp = torch_inputs(cfg, B, T, h, w, 8, dtype=BF)
        assert torch.equal(clone(**inp), model(**inp))
