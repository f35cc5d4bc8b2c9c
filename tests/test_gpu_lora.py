"""GPU: osk_lora_merge_bf16 against its f64 restatement (tests/cpu_ops_lora_f64.py: a derived per-element bound), the MMDiT with
adapters against the oracle run with W + s B A weights, and the plumbing bit for bit.

The issue names the model-level configurations `hd72_eager_split` and `hd128_liger_fused`; oracle/configs.py has no entry of the
second name, so it is built here from `hd128_eager_fused` (the fused head-dim-128 entry) with `use_liger_rope=True`."""
import pytest
import torch

from oracle import configs, mmdit_oracle as O
from tests.cpu_ops_lora_f64 import assert_merged, naive_merge, violates
from tests.lora_util import linear_paths, make_modules, merged_state_dict, write_peft_dir
from tests.util import assert_parity, rel_l2, torch_inputs, torch_params

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _hd128_liger_fused():
    cfg, *geom = configs.GOLDEN["hd128_eager_fused"]
    return (dict(cfg, use_liger_rope=True), *geom)


MODEL_CASES = {"hd72_eager_split": lambda: configs.GOLDEN["hd72_eager_split"], "hd128_liger_fused": _hd128_liger_fused}


# ---------------------------------------------------------------------------------------------- 1. the kernel
def _problem(N, K, ranks, scales, seed, rel=0.3):
    """bf16 W [N, K] ~ N(0, 1 / K) and adapters whose scaled delta has about `rel` of W's Frobenius norm in total"""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF)
    ads = []
    for r, s in zip(ranks, scales):
        a = (torch.randn(r, K, generator=g) * K ** -0.5).to(BF)
        b = torch.randn(N, r, generator=g)
        b = (b * (rel / len(ranks) ** 0.5 * float(w.float().norm()) / float((s * (b @ a.float())).norm()))).to(BF)
        ads.append((a, b, s))
    return w, ads


def _cuda(ads):
    return [(a.cuda(), b.cuda(), s) for a, b, s in ads]


@pytest.mark.parametrize("N,K,r", [(128, 128, 16), (200, 328, 4), (72, 64, 1), (384, 1152, 64), (130, 512, 100), (256, 256, 256)])
def test_merge_matches_f64(hip_lib, N, K, r):
    w, ads = _problem(N, K, [r], [2.0], seed=N + K + r)
    delta = 2.0 * (ads[0][1].double() @ ads[0][0].double())
    assert 0.25 <= float(delta.norm() / w.double().norm()) <= 0.35
    assert violates(naive_merge(w, ads), w, ads)           # a merge that rounds the delta first is told apart at this seed
    out = hip_lib.lora_merge(w.cuda(), torch.empty(N, K, dtype=BF, device="cuda"), _cuda(ads))
    assert_merged(out, w, ads, f"lora_merge [{N} x {K}, r {r}]")


def test_merge_two_adapters_one_rounding(hip_lib):
    N, K = 200, 328
    w, ads = _problem(N, K, [8, 24], [1.5, -0.75], seed=5)
    assert violates(naive_merge(w, ads), w, ads)
    out = hip_lib.lora_merge(w.cuda(), torch.empty(N, K, dtype=BF, device="cuda"), _cuda(ads))
    assert_merged(out, w, ads, "lora_merge, two adapters")


def test_merge_in_place_and_row_slice(hip_lib):
    N, K = 136, 328
    w, ads = _problem(N, K, [12], [-1.25], seed=9)
    ref = hip_lib.lora_merge(w.cuda(), torch.empty(N, K, dtype=BF, device="cuda"), _cuda(ads))
    assert_merged(ref, w, ads, "lora_merge, separate output")
    # out aliasing w
    wd = w.cuda()
    assert hip_lib.lora_merge(wd, wd, _cuda(ads)) is wd and torch.equal(wd, ref)
    # a row-slice / column window inside a larger matrix (row stride > K): nothing outside the window changes its bit pattern
    sentinel = 0x7FC3               # a NaN pattern (int16 view): equality is checked on the bits
    big = torch.full((N + 40, K + 64), sentinel, dtype=torch.int16, device="cuda")
    view = big.view(BF)[24: 24 + N, 16: 16 + K]
    src = torch.full((N + 8, K + 24), sentinel, dtype=torch.int16, device="cuda").view(BF)
    src[8:, 8: 8 + K] = w.cuda()
    hip_lib.lora_merge(src[8:, 8: 8 + K], view, _cuda(ads))
    assert torch.equal(view, ref)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[24: 24 + N, 16: 16 + K] = False
    assert bool((big[mask] == sentinel).all())
    # ... and merged in place inside it
    view.copy_(w.cuda())
    hip_lib.lora_merge(view, view, _cuda(ads))
    assert torch.equal(view, ref) and bool((big[mask] == sentinel).all())


def test_merge_without_adapters_is_a_copy(hip_lib):
    w, _ = _problem(200, 328, [], [], seed=3)
    big = torch.zeros(200, 400, dtype=BF, device="cuda")
    out = hip_lib.lora_merge(w.cuda(), big[:, 8: 8 + 328], [])
    assert torch.equal(out, w.cuda()) and float(big[:, :8].abs().max()) == 0 and float(big[:, 336:].abs().max()) == 0


def test_merge_argument_violations_return_status(hip_lib):
    import ctypes as C

    lib = hip_lib.lib
    N, K, r = 16, 64, 4
    w = torch.zeros(N + 1, K + 8, dtype=BF, device="cuda")
    a = torch.zeros(r, K + 8, dtype=BF, device="cuda")
    b = torch.zeros(N, r, dtype=BF, device="cuda")
    S = K + 8

    def call(w_ptr=w.data_ptr(), ws=S, o_ptr=w.data_ptr(), os_=S, n=N, k=K, n_ad=1, ad_null=False, **ad):
        arr = (hip_lib.OskLoraAdapter * 1)()
        f = dict(a=a.data_ptr(), a_row_stride=S, b=b.data_ptr(), b_row_stride=r, r=r, scale=1.0)
        f.update(ad)
        for key, v in f.items():
            setattr(arr[0], key, v)
        return lib.osk_lora_merge_bf16(w_ptr, ws, o_ptr, os_, n, k, None if ad_null else C.addressof(arr), n_ad, None)

    assert call() == 0
    bad = [dict(w_ptr=None), dict(o_ptr=None), dict(n=0), dict(k=0), dict(k=K + 4), dict(ws=K - 8), dict(os_=K - 8), dict(ws=S + 4),
           dict(os_=S + 4), dict(w_ptr=w.data_ptr() + 2), dict(o_ptr=w.data_ptr() + 8), dict(n_ad=-1), dict(n_ad=9),
           dict(ad_null=True), dict(a=None), dict(b=None), dict(r=0), dict(r=257), dict(a_row_stride=K - 8), dict(a_row_stride=S + 2),
           dict(a=a.data_ptr() + 4), dict(b_row_stride=r - 1), dict(scale=float("nan")), dict(scale=float("inf"))]
    for kw in bad:
        assert call(**kw) < 0, kw
    torch.cuda.synchronize()
    assert float(w.float().abs().max()) == 0


# ---------------------------------------------------------------------------------------------- 2. the model
def _build(cfg):
    from open_sora_amd import mmdit

    model = mmdit.Flux(device_map="cuda", torch_dtype=BF, **cfg)
    model.load_state_dict(torch_params(cfg, dtype=BF, device="cuda"), strict=True)
    return model


_R, _ALPHA = 6, 12.0


@pytest.fixture(scope="module")
def cases():
    """per configuration: the seeded adapter over every Linear kind of both block types (modulation layers included) and the
    oracle's outputs -- computed once, shared by the tests below, never modified"""
    memo = {}

    def get(name):
        if name not in memo:
            cfg, B, T, h, w, L_txt = MODEL_CASES[name]()
            sd32 = torch_params(cfg)
            mods = make_modules(cfg, sd32, 11, _R, _ALPHA)
            assert set(mods) == set(linear_paths(cfg))
            sdm = merged_state_dict(sd32, (mods, _ALPHA / _R))
            with torch.inference_mode():
                truth = O.forward(sdm, cfg, **torch_inputs(cfg, B, T, h, w, L_txt))
                truth_base = O.forward(sd32, cfg, **torch_inputs(cfg, B, T, h, w, L_txt))
                ref_bf16 = O.forward({k: v.bfloat16() for k, v in sdm.items()}, cfg, **torch_inputs(cfg, B, T, h, w, L_txt, dtype=BF))
            memo[name] = dict(cfg=cfg, geom=(B, T, h, w, L_txt), mods=mods, truth=truth, truth_base=truth_base, ref_bf16=ref_bf16)
        return memo[name]

    return get


@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_model_with_adapter_matches_oracle(hip_lib, cases, tmp_path, name):
    from open_sora_amd import lora

    c = cases(name)
    cfg = c["cfg"]
    assert rel_l2(c["truth"], c["truth_base"]) >= 0.1           # the base model cannot pass
    model = _build(cfg)
    lora.load_lora(model, write_peft_dir(tmp_path / "a", c["mods"], _R, _ALPHA))
    inp = torch_inputs(cfg, *c["geom"], dtype=BF, device="cuda")
    with torch.inference_mode():
        out = model(**inp)
    assert_parity(out, c["truth"], c["ref_bf16"], f"MMDiT with LoRA adapter [{name}]")


# ---------------------------------------------------------------------------------------------- 3. the plumbing, bit for bit
def _adapter(lora, mods, r=_R, alpha=_ALPHA):
    return lora.LoraAdapter({p: lora.LoraModule(a, b, r, alpha, alpha / r) for p, (a, b) in mods.items()})


@pytest.mark.parametrize("name,mode", [("hd72_eager_split", "bf16"), ("hd72_eager_split", "fp8"), ("hd128_liger_fused", "bf16"),
                                       ("hd128_liger_fused", "fp8"), ("hd128_liger_fused", "qk8")])
def test_twin_with_merged_state_dict_is_bit_equal(hip_lib, cases, name, mode):
    """a twin whose state dict holds merged_weight(...) of every adapted Linear computes the same bits: the plan feeds the merged
    copies to exactly the kernels the twin runs on its own parameters"""
    from open_sora_amd import lora

    c = cases(name)
    cfg = c["cfg"]
    model, twin = _build(cfg), _build(cfg)
    lora.load_lora(model, _adapter(lora, c["mods"]))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    for p in c["mods"]:
        merged = lora.merged_weight(model, p)
        assert not torch.equal(merged, sd[p + ".weight"])
        sd[p + ".weight"] = merged.clone()
    twin.load_state_dict(sd, strict=True)
    if mode != "bf16":
        model.enable_fp8(qk8=(mode == "qk8"))
        twin.enable_fp8(qk8=(mode == "qk8"))
    inp = torch_inputs(cfg, *c["geom"], dtype=BF, device="cuda")
    with torch.inference_mode():
        assert torch.equal(model(**inp), twin(**inp))


def test_weight_zero_and_unload_restore_the_base_model(hip_lib, cases):
    from open_sora_amd import lora

    c = cases("hd72_eager_split")
    cfg = c["cfg"]
    model = _build(cfg)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    inp = torch_inputs(cfg, *c["geom"], dtype=BF, device="cuda")
    with torch.inference_mode():
        base = model(**inp).clone()
        lora.load_lora(model, _adapter(lora, c["mods"]), name="a")
        assert not torch.equal(model(**inp), base)
        lora.set_lora_weights(model, {"a": 0.0})
        assert torch.equal(model(**inp), base)
        lora.set_lora_weights(model, {"a": 1.0})
        assert not torch.equal(model(**inp), base)
        lora.unload_lora(model, "a")
        assert torch.equal(model(**inp), base)
    assert all(torch.equal(v, sd0[k]) for k, v in model.state_dict().items())


def test_two_adapters_equal_one_kernel_call_with_both(hip_lib, cases):
    from open_sora_amd import lora

    c = cases("hd72_eager_split")
    cfg = c["cfg"]
    sd32 = torch_params(cfg)
    paths = ["double_blocks.0.img_attn.k_proj", "single_blocks.1.v_mlp", "double_blocks.0.txt_mod.lin"]
    m1 = make_modules(cfg, sd32, 21, 8, 16.0, paths=paths)
    m2 = make_modules(cfg, sd32, 22, 24, 6.0, paths=paths[:2])
    model = _build(cfg)
    lora.load_lora(model, _adapter(lora, m1, 8, 16.0), name="one", weight=0.5)
    lora.load_lora(model, _adapter(lora, m2, 24, 6.0), name="two", weight=1.0)
    for p in paths[:2]:
        w = model.get_submodule(p).weight.detach()
        ads = [(m1[p][0].to(BF).cuda(), m1[p][1].to(BF).cuda(), 0.5 * 16.0 / 8), (m2[p][0].to(BF).cuda(), m2[p][1].to(BF).cuda(), 1.0 * 6.0 / 24)]
        one_call = hip_lib.lora_merge(w, torch.empty_like(w), ads)
        assert torch.equal(lora.merged_weight(model, p), one_call), p
        assert_merged(one_call, w, ads, f"two adapters on {p}")
