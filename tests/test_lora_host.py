"""CPU: the host side of the LoRA support (open_sora_amd/lora.py and the plan hooks of mmdit.py) on the CPU emulation of the
kernels (tests/cpu_ops.py has no `lora_merge`: the torch-f32 arithmetic of mmdit._lora_merge runs).  Adapter directories are written
here, in peft's documented on-disk format, with `json` and `safetensors` only."""
import os

import pytest
import torch

from oracle import configs, mmdit_oracle as O
from tests import cpu_ops
from tests.cpu_ops_lora_f64 import assert_merged
from tests.lora_util import linear_paths, make_modules, merged_state_dict, write_peft_dir
from tests.util import assert_parity, rel_l2, torch_inputs, torch_params

BF = torch.bfloat16
FUSED, SPLIT = "hd64_eager_fused", "hd64_liger_split"


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


def _expected(w: torch.Tensor, *terms) -> torch.Tensor:
    """bf16(W + sum s B A) in f64: what one rounding of the exact sum gives.  The f32 arithmetic under test may differ from it by
    one bf16 step where the exact value sits within f32 noise of a rounding boundary: merged weights are judged with the criterion
    of tests/cpu_ops_lora_f64.py (assert_merged), this value only serves to show that two results are NOT the same."""
    acc = w.double()
    for a, b, s in terms:
        acc = acc + s * (b.double() @ a.double())
    return acc.to(BF)


# ---------------------------------------------------------------------------------------------- reading
def test_scale_rules(tmp_path):
    from open_sora_amd import lora

    cfg = configs.GOLDEN[FUSED][0]
    sd32 = torch_params(cfg)
    p4, p8 = "double_blocks.0.img_attn.proj", "single_blocks.1.linear2"
    mods = make_modules(cfg, sd32, 0, 4, 8.0, paths=[p4, "double_blocks.1.img_attn.proj"])
    mods.update(make_modules(cfg, sd32, 1, 8, 8.0, paths=[p8]))
    # alpha / r, with rank_pattern (suffix rule: `single_blocks.1.linear2` and bare `linear2` both match) and alpha_pattern
    d = write_peft_dir(tmp_path / "a", mods, 4, 8.0, rank_pattern={"single_blocks.1.linear2": 8}, alpha_pattern={"0.img_attn.proj": 2.0})
    ad = lora.read_peft_adapter(d)
    assert set(ad.modules) == set(mods)
    assert (ad.modules[p8].r, ad.modules[p8].scale) == (8, 8.0 / 8)
    assert (ad.modules[p4].r, ad.modules[p4].alpha, ad.modules[p4].scale) == (4, 2.0, 2.0 / 4)
    m = ad.modules["double_blocks.1.img_attn.proj"]          # `0.img_attn.proj` must not match `double_blocks.1.img_attn.proj`
    assert (m.r, m.alpha, m.scale) == (4, 8.0, 8.0 / 4)
    assert torch.equal(m.a, mods["double_blocks.1.img_attn.proj"][0]) and torch.equal(m.b, mods["double_blocks.1.img_attn.proj"][1])
    d = write_peft_dir(tmp_path / "b", mods, 4, 8.0, rank_pattern={"linear2": 8})
    assert lora.read_peft_adapter(d).modules[p8].r == 8
    # rslora: alpha / sqrt(r)
    d = write_peft_dir(tmp_path / "c", mods, 4, 8.0, rank_pattern={"linear2": 8}, use_rslora=True)
    ad = lora.read_peft_adapter(d)
    assert ad.modules[p4].scale == 8.0 / 2.0 and ad.modules[p8].scale == 8.0 / 8 ** 0.5
    # adapter_model.bin when the safetensors file is absent
    d = write_peft_dir(tmp_path / "d", mods, 4, 8.0, fmt="bin", rank_pattern={"linear2": 8})
    assert not os.path.exists(os.path.join(d, "adapter_model.safetensors"))
    ad = lora.read_peft_adapter(d)
    assert torch.equal(ad.modules[p8].b, mods[p8][1]) and ad.modules[p4].scale == 2.0


@pytest.mark.parametrize("field,config", [("peft_type", dict(peft_type="LOHA")), ("use_dora", dict(use_dora=True)),
                                          ("bias", dict(bias="all")), ("bias", dict(bias="lora_only")),
                                          ("fan_in_fan_out", dict(fan_in_fan_out=True)),
                                          ("modules_to_save", dict(modules_to_save=["final_layer"]))])
def test_refused_config_fields(tmp_path, field, config):
    from open_sora_amd import lora

    cfg = configs.GOLDEN[FUSED][0]
    mods = make_modules(cfg, torch_params(cfg), 0, 4, 4.0, paths=["double_blocks.0.img_attn.proj"])
    d = write_peft_dir(tmp_path / "a", mods, 4, 4.0, **config)
    with pytest.raises(ValueError, match=field):
        lora.read_peft_adapter(d)


def test_refused_keys_and_shapes(cpu_mmdit, tmp_path):
    from open_sora_amd import lora

    cfg = configs.GOLDEN[FUSED][0]
    model = _build(cpu_mmdit, cfg)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    D = cfg["hidden_size"]
    a, b = torch.zeros(4, D), torch.zeros(D, 4)
    bad = {
        "outside the blocks": {"img_in": (torch.zeros(4, cfg["in_channels"]), b)},
        "final layer": {"final_layer.linear": (a, torch.zeros(cfg["in_channels"], 4))},
        "not a Linear": {"double_blocks.0.img_attn": (a, b)},
        "no such module": {"double_blocks.0.img_attn.q_proj": (a, b)},          # the fused model has `qkv`
        "in features": {"double_blocks.0.img_attn.proj": (torch.zeros(4, D + 8), b)},
        "out features": {"double_blocks.0.img_attn.proj": (a, torch.zeros(D + 8, 4))},
        "rank of A": {"double_blocks.0.img_attn.proj": (torch.zeros(8, D), b)},
    }
    for i, (what, mods) in enumerate(bad.items()):
        d = write_peft_dir(tmp_path / f"k{i}", mods, 4, 4.0)
        with pytest.raises(ValueError, match="adapter key"):
            lora.load_lora(model, d, name=f"k{i}")
        assert lora.lora_report(model) == [], what
    # a tensor that is neither lora_A nor lora_B (a DoRA magnitude, an embedding adapter)
    from safetensors.torch import save_file

    d = write_peft_dir(tmp_path / "m", {"double_blocks.0.img_attn.proj": (a, b)}, 4, 4.0)
    save_file({"base_model.model.double_blocks.0.img_attn.proj.lora_magnitude_vector": torch.zeros(D)},
              os.path.join(d, "adapter_model.safetensors"))
    with pytest.raises(ValueError, match="adapter key"):
        lora.read_peft_adapter(d)
    assert all(torch.equal(v, sd0[k]) for k, v in model.state_dict().items())


# ---------------------------------------------------------------------------------------------- merging
@pytest.mark.parametrize("name", [FUSED, SPLIT])
def test_qkv_keys_map_onto_the_concatenated_rows(cpu_mmdit, tmp_path, name):
    """fused checkpoints adapt `qkv` / `linear1` as a whole; split ones q_proj | k_proj | v_proj (v_mlp) piece by piece: each lands in
    its row slice of the plan's concatenated weight, an un-adapted piece keeps the base rows"""
    from open_sora_amd import lora

    cfg = configs.GOLDEN[name][0]
    model = _build(cpu_mmdit, cfg)
    sd32 = torch_params(cfg)
    D = cfg["hidden_size"]
    if cfg["fused_qkv"]:
        paths = ["double_blocks.0.img_attn.qkv", "single_blocks.0.linear1"]
    else:
        paths = ["double_blocks.0.img_attn.k_proj", "double_blocks.0.txt_attn.q_proj", "double_blocks.0.txt_attn.v_proj",
                 "single_blocks.0.k_proj", "single_blocks.0.v_mlp"]
    mods = make_modules(cfg, sd32, 3, 4, 8.0, paths=paths)
    lora.load_lora(model, write_peft_dir(tmp_path / "a", mods, 4, 8.0))
    exp = {p: lora.merged_weight(model, p) for p in paths}
    for p, (a, b) in mods.items():
        assert_merged(exp[p], sd32[p + ".weight"], [(a, b, 2.0)], p)
        assert not torch.equal(exp[p], sd32[p + ".weight"].to(BF))
    pd, ps = cpu_mmdit.plan_double(model.double_blocks[0]), cpu_mmdit.plan_single(model.single_blocks[0])
    base = lambda p: sd32[p + ".weight"].to(BF)
    if cfg["fused_qkv"]:
        assert torch.equal(pd.img.qkv_w, exp[paths[0]]) and torch.equal(ps.w1, exp[paths[1]])
        assert torch.equal(pd.txt.qkv_w, base("double_blocks.0.txt_attn.qkv"))
        assert pd.txt.qkv_w.data_ptr() == model.double_blocks[0].txt_attn.qkv.weight.data_ptr()      # un-adapted: today's zero-copy view
    else:
        pre = "double_blocks.0."
        assert torch.equal(pd.img.qkv_w, torch.cat([base(pre + "img_attn.q_proj"), exp[pre + "img_attn.k_proj"], base(pre + "img_attn.v_proj")]))
        assert torch.equal(pd.txt.qkv_w, torch.cat([exp[pre + "txt_attn.q_proj"], base(pre + "txt_attn.k_proj"), exp[pre + "txt_attn.v_proj"]]))
        assert torch.equal(ps.w1, torch.cat([base("single_blocks.0.q_proj"), exp["single_blocks.0.k_proj"], exp["single_blocks.0.v_mlp"]]))
        assert ps.w1.shape[0] == 3 * D + int(D * cfg["mlp_ratio"])
    assert pd.img.proj_w.data_ptr() == model.double_blocks[0].img_attn.proj.weight.data_ptr()


def test_two_adapters_on_one_linear_round_once(cpu_mmdit):
    from open_sora_amd import lora

    cfg = configs.GOLDEN[FUSED][0]
    model = _build(cpu_mmdit, cfg)
    sd32 = torch_params(cfg)
    p, q = "double_blocks.1.txt_mlp.0", "single_blocks.2.modulation.lin"
    m1 = make_modules(cfg, sd32, 1, 8, 16.0, paths=[p, q])
    m2 = make_modules(cfg, sd32, 2, 24, 12.0, paths=[p])
    mk = lambda mods, r, alpha: lora.LoraAdapter({k: lora.LoraModule(a, b, r, alpha, alpha / r) for k, (a, b) in mods.items()})
    lora.load_lora(model, mk(m1, 8, 16.0), name="one", weight=0.5)
    lora.load_lora(model, mk(m2, 24, 12.0), name="two", weight=-1.0)
    w = sd32[p + ".weight"]
    both = _expected(w, (*m1[p], 0.5 * 2.0), (*m2[p], -1.0 * 0.5))
    assert_merged(lora.merged_weight(model, p), w, [(*m1[p], 0.5 * 2.0), (*m2[p], -1.0 * 0.5)], "two adapters")
    twice = _expected(_expected(w, (*m1[p], 1.0)).float(), (*m2[p], -0.5))     # rounding after each adapter is NOT the same thing
    assert not torch.equal(twice, both)
    rep = lora.lora_report(model)
    assert [(r["name"], r["weight"]) for r in rep] == [("one", 0.5), ("two", -1.0)]
    assert rep[0]["modules"] == {p: {"r": 8, "scale": 2.0}, q: {"r": 8, "scale": 2.0}} and rep[1]["modules"] == {p: {"r": 24, "scale": 0.5}}
    with pytest.raises(ValueError, match="already loaded"):
        lora.load_lora(model, mk(m2, 24, 12.0), name="two")
    lora.set_lora_weights(model, {"two": 0.0})
    assert_merged(lora.merged_weight(model, p), w, [(*m1[p], 1.0)], "second adapter at weight 0")
    lora.unload_lora(model, "one")
    assert lora.merged_weight(model, p).data_ptr() == model.get_submodule(p).weight.data_ptr()      # weight 0: the zero-copy view again
    assert torch.equal(lora.merged_weight(model, q), sd32[q + ".weight"].to(BF))
    with pytest.raises(KeyError):
        lora.unload_lora(model, "one")
    with pytest.raises(KeyError):
        lora.set_lora_weights(model, {"nobody": 1.0})


def test_state_dict_untouched_and_plan_rebuilt_only_on_adapter_changes(cpu_mmdit, tmp_path, monkeypatch):
    from open_sora_amd import lora

    cfg, B, T, h, w, L_txt = configs.GOLDEN[SPLIT]
    model = _build(cpu_mmdit, cfg)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    ptrs = {k: v.data_ptr() for k, v in model.state_dict().items()}
    builds = []
    orig = cpu_mmdit.MMDiTModel._build_plan
    monkeypatch.setattr(cpu_mmdit.MMDiTModel, "_build_plan", lambda self, dev: (builds.append(1), orig(self, dev))[1])
    inp = torch_inputs(cfg, B, T, h, w, L_txt, dtype=BF)
    d = write_peft_dir(tmp_path / "a", make_modules(cfg, torch_params(cfg), 5, 4, 4.0), 4, 4.0)

    def run(expect_builds):
        with torch.inference_mode():
            out = model(**inp)
            assert len(builds) == expect_builds
            assert torch.equal(model(**inp), out) and len(builds) == expect_builds      # a second forward never rebuilds
        return out

    base = run(1)
    lora.load_lora(model, d, name="a")
    with_a = run(2)
    assert lora.lora_report(model)[0]["name"] == "a" and len(builds) == 2                # reporting plans nothing
    lora.merged_weight(model, "single_blocks.0.v_mlp")
    run(2)                                                                                   # ... and neither does merged_weight
    lora.set_lora_weights(model, {"a": 0.5})
    half = run(3)
    lora.set_lora_weights(model, {"a": 1.0})
    assert torch.equal(run(4), with_a)
    lora.unload_lora(model)
    assert torch.equal(run(5), base)
    assert not torch.equal(with_a, base) and not torch.equal(half, with_a) and not torch.equal(half, base)
    sd1 = model.state_dict()
    assert list(sd1) == list(sd0) and all(torch.equal(sd1[k], sd0[k]) and sd1[k].data_ptr() == ptrs[k] for k in sd0)


@pytest.mark.parametrize("name", [FUSED, SPLIT])
def test_forward_with_adapter_follows_the_oracle(cpu_mmdit, tmp_path, name):
    """every Linear kind of both block types adapted (modulation layers included): the forward follows the oracle run with
    W + s B A weights; after unload_lora it is the forward before loading, bit for bit"""
    from open_sora_amd import lora

    cfg, B, T, h, w, L_txt = configs.GOLDEN[name]
    model = _build(cpu_mmdit, cfg)
    sd32 = torch_params(cfg)
    r, alpha = 6, 12.0
    mods = make_modules(cfg, sd32, 11, r, alpha)
    assert set(mods) == set(linear_paths(cfg))
    sdm = merged_state_dict(sd32, (mods, alpha / r))
    inp = torch_inputs(cfg, B, T, h, w, L_txt, dtype=BF)
    with torch.inference_mode():
        before = model(**inp)
        lora.load_lora(model, write_peft_dir(tmp_path / "a", mods, r, alpha))
        out = model(**inp)
        truth = O.forward(sdm, cfg, **torch_inputs(cfg, B, T, h, w, L_txt))
        truth_base = O.forward(sd32, cfg, **torch_inputs(cfg, B, T, h, w, L_txt))
        ref_bf16 = O.forward({k: v.bfloat16() for k, v in sdm.items()}, cfg, **inp)
        assert rel_l2(truth, truth_base) >= 0.1          # the base model cannot pass
        assert_parity(out, truth, ref_bf16, f"CPU emulation with adapter [{name}]")
        lora.unload_lora(model)
        assert torch.equal(model(**inp), before)


def test_fp8_mode_wraps_the_merged_weight(cpu_mmdit):
    """adapters and enable_fp8 compose in either order: the fp8 plan quantises the merged bf16 weight"""
    from open_sora_amd import lora

    cfg = configs.GOLDEN[FUSED][0]
    sd32 = torch_params(cfg)
    p = "double_blocks.0.img_mlp.2"
    mods = make_modules(cfg, sd32, 4, 4, 4.0, paths=[p])
    ad = lora.LoraAdapter({k: lora.LoraModule(a, b, 4, 4.0, 1.0) for k, (a, b) in mods.items()})
    plans = []
    for order in (0, 1):
        model = _build(cpu_mmdit, cfg)
        steps = [lambda: model.enable_fp8(), lambda: lora.load_lora(model, ad)]
        for s in (steps if order == 0 else steps[::-1]):
            s()
        plans.append(cpu_mmdit.plan_double(model.double_blocks[0]).img_mlp[2])
    for w in plans:
        assert isinstance(w, cpu_mmdit.Fp8Weight)
        assert_merged(w.w, sd32[p + ".weight"], [(*mods[p], 1.0)], "fp8 mode: bf16 rows")
    assert torch.equal(plans[0].w, plans[1].w) and torch.equal(plans[0].w8, plans[1].w8) and torch.equal(plans[0].sw, plans[1].sw)
    assert torch.equal(plans[0].w8, cpu_ops.quantize_rows_fp8(plans[0].w)[0])
