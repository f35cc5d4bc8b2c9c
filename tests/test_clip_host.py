"""CPU: host side of the CLIP text encoder (open_sora_amd.clip), driven through the CPU emulation of the kernels' semantics
(tests/cpu_ops_clip.py), and the plain-torch restatement the GPU tests take as truth (tests/clip_restatement.py) pinned to the output
transformers itself produced (tests/golden/clip_small.npz, recorded by tools/make_golden_clip.py) and, where transformers imports, to
the live model.  The kernels themselves are checked on the GPU by tests/test_gpu_clip.py."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests import clip_restatement as R
from tests import cpu_ops_clip
from tests.util import assert_parity, finite_retry, rel_l2
from tools.make_golden_clip import EOS_AT, input_ids, small_state_dict

BF = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_small.npz")
TOP = R.SMALL["vocab_size"] - 1


@pytest.fixture()
def emu(hip_lib):
    from open_sora_amd import clip, mmdit

    mmdit.set_ops_for_testing(cpu_ops_clip)
    yield clip
    mmdit.set_ops_for_testing(hip_lib)


@pytest.fixture(scope="module")
def golden():
    return {k: v for k, v in np.load(GOLDEN).items()}


def small_model(C, dtype=BF, **cfg):
    m = C.ClipTextModel(C.ClipTextConfig(**{**R.SMALL, **cfg})).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in small_state_dict().items()})
    return m


def restated(ids, dtype=torch.float32, **cfg):
    sd = {k: v.to(dtype) for k, v in small_state_dict().items()}
    with torch.no_grad():
        return R.encode(sd, {**R.SMALL, **cfg}, ids)


# ------------------------------------------------------------------------------------------------ restatement == transformers
def test_restatement_matches_golden(golden):
    ids = torch.from_numpy(golden["input_ids"])
    assert torch.equal(ids, input_ids()), "the seeded generator no longer reproduces the recorded input_ids"
    y, pooled = restated(ids)
    want, want_p = torch.from_numpy(golden["last_hidden_state"]), torch.from_numpy(golden["pooler_output"])
    assert y.shape == want.shape == (3, 77, 128) and pooled.shape == want_p.shape == (3, 128)
    assert rel_l2(y, want) <= 1e-5 and rel_l2(pooled, want_p) <= 1e-5, (rel_l2(y, want), rel_l2(pooled, want_p))   # fp32 round-off of 3 layers


def test_restatement_bf16_is_a_fair_comparator(golden):
    """the restatement's bf16 run rounds where transformers' bf16 run rounds: the two are equally far from the fp32 output"""
    want = torch.from_numpy(golden["last_hidden_state"])
    hf16 = torch.from_numpy(golden["last_hidden_state_bf16_bits"]).view(BF)
    ours16 = finite_retry(lambda: restated(torch.from_numpy(golden["input_ids"]), BF)[0])
    e_hf, e_re = rel_l2(hf16, want), rel_l2(ours16, want)
    assert 0.5 * e_hf <= e_re <= 2.0 * e_hf, (e_hf, e_re)


def test_restatement_matches_live_transformers():
    pytest.importorskip("transformers")
    from tools.make_golden_clip import hf_model, hf_outputs

    sd = small_state_dict()
    g = torch.Generator().manual_seed(5)
    for eos, shape in ((2, (1, 7)), (2, (2, 65)), (300, (4, 77))):
        m = hf_model({**R.SMALL, "eos_token_id": eos}, sd)
        ids = torch.randint(0, R.SMALL["vocab_size"], shape, generator=g)
        ids[:, -2] = eos                                                  # every row holds the token the second convention looks for
        (y, pooled), (want, want_p) = restated(ids, eos_token_id=eos), hf_outputs(m, ids)
        assert rel_l2(y, want) <= 1e-5 and rel_l2(pooled, want_p) <= 1e-5, (eos, shape)


# --------------------------------------------------------------------------------------------------------- state dict
def test_state_dict_keys_match_the_fixture(emu, golden):
    want = [str(k) for k in golden["keys"]]
    sd = small_model(emu).state_dict()
    assert list(sd) == want == list(small_state_dict()) == list(R.param_shapes(R.SMALL))
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v) for k, v in R.param_shapes(R.SMALL).items()}
    assert not any(k.startswith("text_model.") for k in want) and "embeddings.position_ids" not in want


def test_clip_l_preset_keys_and_shapes(emu):
    cfg = emu.ClipTextConfig.clip_vit_l_14()
    assert (cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
            cfg.max_position_embeddings, cfg.layer_norm_eps, cfg.eos_token_id) == (49408, 768, 3072, 12, 12, 77, 1e-5, 2)
    with torch.device("meta"):
        m = emu.ClipTextModel(cfg)
    shapes = R.param_shapes(dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                                 max_position_embeddings=77))
    sd = m.state_dict()
    assert list(sd) == list(shapes) and {k: tuple(v.shape) for k, v in sd.items()} == shapes
    assert sum(p.numel() for p in m.parameters()) == 123_060_480


def test_load_state_dict_accepts_the_text_model_prefix_and_is_strict(emu):
    sd = small_state_dict()
    m = emu.ClipTextModel(emu.ClipTextConfig(**R.SMALL))
    prefixed = {"text_model." + k: v for k, v in sd.items()}
    prefixed["text_model.embeddings.position_ids"] = torch.arange(77)[None]          # the buffer transformers 4 checkpoints store
    m.load_state_dict(prefixed, strict=True)
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    plain = dict(sd)
    plain["embeddings.position_ids"] = torch.arange(77)[None]
    emu.ClipTextModel(emu.ClipTextConfig(**R.SMALL)).load_state_dict(plain, strict=True)
    short = dict(prefixed)
    short.pop("text_model.encoder.layers.1.mlp.fc1.bias")
    with pytest.raises(RuntimeError, match="fc1.bias"):
        m.load_state_dict(short)
    extra = dict(sd)
    extra["text_projection.weight"] = torch.zeros(4, 128)
    with pytest.raises(RuntimeError, match="text_projection"):
        m.load_state_dict(extra)


def test_from_hf_module_round_trips(emu):
    pytest.importorskip("transformers")
    from tools.make_golden_clip import hf_model, hf_outputs

    sd = small_state_dict()
    hf = hf_model(R.SMALL, sd, BF)
    m = emu.ClipTextModel.from_hf_module(hf)
    assert m.cfg == emu.ClipTextConfig(**R.SMALL) and m.dtype == BF and not m.training
    got, want = m.state_dict(), hf.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    hf.load_state_dict(got, strict=True)                            # and back
    ids = input_ids()[:, :40]
    out = m(input_ids=ids, attention_mask=None, output_hidden_states=False)
    y32, p32 = restated(ids)
    y16, p16 = restated(ids, BF)
    assert_parity(out["last_hidden_state"], y32, y16, "from_hf_module forward, last_hidden_state")
    assert_parity(out["pooler_output"], p32, p16, "from_hf_module forward, pooler_output")
    hf32 = hf_model(R.SMALL, sd)
    assert rel_l2(hf_outputs(hf32, ids)[0], y32) <= 1e-5            # and the live model is what the restatement says


def test_from_hf_module_refuses_another_activation(emu):
    pytest.importorskip("transformers")
    from tools.make_golden_clip import hf_model

    hf = hf_model(dict(R.SMALL, num_hidden_layers=1), None, hidden_act="gelu")
    with pytest.raises(ValueError, match="hidden_act 'gelu'"):
        emu.ClipTextModel.from_hf_module(hf)


def test_unsupported_configurations_are_refused_at_construction(emu):
    for change, match in ((dict(hidden_act="gelu"), "hidden_act 'gelu'"), (dict(num_attention_heads=4), "head dim 32"),
                          (dict(intermediate_size=520), "intermediate_size 520"), (dict(hidden_size=200, num_attention_heads=3), "head dim"),
                          (dict(num_hidden_layers=0), "num_hidden_layers")):
        with pytest.raises(ValueError, match=match):
            emu.ClipTextModel(emu.ClipTextConfig(**{**R.SMALL, **change}))


# ------------------------------------------------------------------------------------- the encoder through the emulated kernels
def test_emulated_forward_matches_restatement_and_golden(emu, golden):
    ids = torch.from_numpy(golden["input_ids"])
    m = small_model(emu, torch.float32)
    out = m(input_ids=ids, attention_mask=None, output_hidden_states=False)
    assert out["last_hidden_state"] is out.last_hidden_state and list(out) == ["last_hidden_state", "pooler_output"]
    y, pooled = out.last_hidden_state, out["pooler_output"]
    assert y.dtype == pooled.dtype == torch.float32 and tuple(y.shape) == (3, 77, 128) and tuple(pooled.shape) == (3, 128)
    y32, p32 = restated(ids)
    y16, p16 = restated(ids, BF)
    assert_parity(y, y32, y16, "emulated CLIP text encoder vs restatement")
    assert_parity(pooled, p32, p16, "emulated CLIP pooler_output vs restatement")
    assert_parity(y, torch.from_numpy(golden["last_hidden_state"]), torch.from_numpy(golden["last_hidden_state_bf16_bits"]).view(BF),
                  "emulated CLIP text encoder vs transformers' recorded output")
    assert_parity(pooled, torch.from_numpy(golden["pooler_output"]), torch.from_numpy(golden["pooler_output_bf16_bits"]).view(BF),
                  "emulated CLIP pooler_output vs transformers' recorded output")
    assert all(torch.equal(pooled[b], y[b, at]) for b, at in enumerate(EOS_AT))
    assert torch.equal(m(ids).last_hidden_state, y)                 # the cached plan and workspace: bit-identical


def test_pooling_takes_the_largest_id_when_eos_is_2(emu):
    m = small_model(emu)
    ids = torch.randint(0, TOP, (3, 77), generator=torch.Generator().manual_seed(8))
    where = (0, 10, 76)
    for b, at in enumerate(where):
        ids[b, at] = TOP
    out = m(ids)
    assert all(torch.equal(out.pooler_output[b], out.last_hidden_state[b, at]) for b, at in enumerate(where))


def test_pooling_takes_the_first_eos_otherwise(emu):
    eos, bos = TOP, 7
    m = small_model(emu, eos_token_id=eos)
    ids = torch.randint(0, TOP, (2, 30), generator=torch.Generator().manual_seed(9))
    ids[0, 12] = ids[0, 20] = eos                                   # twice in a row: the first occurrence wins
    ids[1] = eos
    ids[1, 0] = bos                                                 # [bos, eos, eos, ...]
    out = m(ids)
    assert torch.equal(out.pooler_output[0], out.last_hidden_state[0, 12])
    assert torch.equal(out.pooler_output[1], out.last_hidden_state[1, 1])
    assert_parity(out.pooler_output, restated(ids, eos_token_id=eos)[1], restated(ids, BF, eos_token_id=eos)[1], "pooler_output, eos 511")


def test_ids_behind_the_pooled_position_do_not_reach_pooler_output(emu):
    """causality end to end: the pooled row sees the tokens up to its own position only"""
    m = small_model(emu)
    g = torch.Generator().manual_seed(10)
    ids = torch.randint(0, TOP, (3, 77), generator=g)
    where = (0, 10, 63)
    for b, at in enumerate(where):
        ids[b, at] = TOP
    first = m(ids).pooler_output.clone()
    other = ids.clone()
    for b, at in enumerate(where):
        other[b, at + 1:] = torch.randint(0, TOP, (77 - at - 1,), generator=g)
    assert not torch.equal(other, ids)
    out = m(other)
    assert torch.equal(out.pooler_output, first)
    assert not torch.equal(out.last_hidden_state, m(ids).last_hidden_state)


def test_forward_runs_only_kernel_table_ops_in_the_documented_order(emu):
    calls = []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(cpu_ops_clip, name)

            def op(*a, **k):
                calls.append(name)
                return fn(*a, **k)
            return op

    from open_sora_amd import mmdit

    m = small_model(emu)
    mmdit.set_ops_for_testing(Spy())
    try:
        m(input_ids()[:, :16])
    finally:
        mmdit.set_ops_for_testing(cpu_ops_clip)
    layer = ["layernorm_affine", "gemm", "attention_causal", "gemm", "layernorm_affine", "gemm_quickgelu", "gemm"]
    assert len(layer) == 7 and calls == layer * 3 + ["layernorm_affine"]


def test_sequence_lengths(emu):
    m = small_model(emu)
    ids = torch.randint(0, TOP, (2, 20), generator=torch.Generator().manual_seed(20))
    out = m(ids)
    y32, _ = restated(ids)
    assert tuple(out.last_hidden_state.shape) == (2, 20, 128)
    assert_parity(out.last_hidden_state, y32, finite_retry(lambda: restated(ids, BF)[0]), "emulated CLIP text encoder L = 20")
    with pytest.raises(ValueError, match="78 tokens exceed max_position_embeddings 77"):
        m(torch.zeros(1, 78, dtype=torch.long))


def test_attention_mask_is_refused(emu):
    m = small_model(emu)
    ids = input_ids()[:, :8]
    with pytest.raises(ValueError, match="attention_mask=None"):
        m(input_ids=ids, attention_mask=torch.ones_like(ids))
    m(input_ids=ids, attention_mask=None, output_hidden_states=False, return_dict=True)      # further keywords are ignored


def test_plan_follows_the_parameters(emu):
    m = small_model(emu)
    ids = input_ids()[:, :24]
    y0 = m(ids).last_hidden_state
    assert m._plan() is m._plan()
    sd = small_state_dict()
    sd["final_layer_norm.weight"] = sd["final_layer_norm.weight"] * 2
    sd["final_layer_norm.bias"] = sd["final_layer_norm.bias"] * 2
    m.load_state_dict({k: v.to(BF) for k, v in sd.items()})
    assert rel_l2(m(ids).last_hidden_state, 2 * y0.float()) <= 2.0 ** -7           # load_state_dict dropped the plan
    with torch.no_grad():
        m.final_layer_norm.weight.mul_(0.5)                         # an in-place update is seen through the version counter
        m.final_layer_norm.bias.mul_(0.5)
    assert rel_l2(m(ids).last_hidden_state, y0) <= 2.0 ** -7
    p = m._plan()
    m.invalidate_plan()
    assert m._plan() is not p


# ------------------------------------------------------------------------------------------------------------ ClipEmbedder
class _StubTokenizer:
    pad_token_id = 3

    def __init__(self, n_tokens):
        self.n_tokens, self.calls = n_tokens, []

    def __call__(self, text, **kw):
        self.calls.append((list(text), kw))
        ids = torch.arange(1, self.n_tokens + 1).repeat(len(text), 1) % 100 + 4
        ids[:, -1] = TOP
        return {"input_ids": ids}


class _StubEncoder(torch.nn.Module):
    device = torch.device("cpu")

    def forward(self, input_ids, attention_mask="unset", **kw):
        self.seen = (input_ids.clone(), attention_mask, kw)
        return {"pooler_output": input_ids[:, :1].float(), "last_hidden_state": input_ids[..., None].float()}


@pytest.mark.parametrize("n_tokens,added,align,want", [(77, 0, 1, 77), (77, 0, 7, 77), (77, 0, 8, 80), (77, 3, 8, 77), (77, 4, 8, 84),
                                                       (20, 1, 64, 63)])
def test_embedder_reproduces_the_seq_align_padding(emu, n_tokens, added, align, want):
    tok, enc = _StubTokenizer(n_tokens), _StubEncoder()
    e = emu.ClipEmbedder(tok, enc, max_length=n_tokens)
    out = e(["a prompt", ""], added_tokens=added, seq_align=align)
    ids, mask, kw = enc.seen
    assert tuple(ids.shape) == (2, want) and (added + want) % align == 0 and tuple(out.shape) == (2, 1)
    assert torch.equal(ids[:, :n_tokens], tok(["a", "b"])["input_ids"]) and bool((ids[:, n_tokens:] == tok.pad_token_id).all())
    assert mask is None and kw == {"output_hidden_states": False}
    text, call = tok.calls[0]
    assert text == ["a prompt", ""]
    assert call == dict(truncation=True, max_length=n_tokens, return_length=False, return_overflowing_tokens=False,
                        padding="max_length", return_tensors="pt")
    assert e.output_key == "pooler_output" and e.hf_module is enc and e.is_clip is True
    assert list(inspect.signature(e.forward).parameters) == ["text", "added_tokens", "seq_align"]
    assert [p.default for p in inspect.signature(e.forward).parameters.values()][1:] == [0, 1]


def test_embedder_around_the_emulated_encoder(emu):
    m = small_model(emu)
    e = emu.ClipEmbedder(_StubTokenizer(20), m, max_length=20)
    y = e(["x", "y"], seq_align=16)
    ids = torch.nn.functional.pad(_StubTokenizer(20)(["x", "y"])["input_ids"], (0, 12), value=3)
    assert tuple(y.shape) == (2, 128) and torch.equal(y, m(ids).pooler_output) and torch.equal(y, m(ids).last_hidden_state[:, 19])


# ------------------------------------------------------------------------------------------------------- the emulation itself
def test_emulated_ops_match_torch():
    g = torch.Generator().manual_seed(2)
    B, L, H = 2, 70, 3
    q, k, v = (torch.randn(B, L, H * 64, generator=g) for _ in range(3))
    want = R.attention(*(t.double().view(B, L, H, 64) for t in (q, k, v)), 0.125).reshape(B, L, H * 64)
    assert rel_l2(cpu_ops_clip.attention_causal_ref(q, k, v, H, 64, 0.125, dtype=torch.float64), want) <= 1e-6
    full = torch.nn.functional.scaled_dot_product_attention(*(t.double().view(B, L, H, 64).transpose(1, 2) for t in (q, k, v)), is_causal=True)
    assert rel_l2(want, full.transpose(1, 2).reshape(B, L, H * 64)) <= 1e-6           # (the restatement's softmax is f32)
    x, w, b = torch.randn(5, 128, generator=g) * 3 + 7, torch.randn(128, generator=g), torch.randn(128, generator=g)
    assert rel_l2(cpu_ops_clip.layernorm_affine_ref(x, w, b, 1e-5), torch.nn.functional.layer_norm(x, (128,), w, b, 1e-5)) <= 1e-6
    a, wt = torch.randn(9, 64, generator=g), torch.randn(24, 64, generator=g)
    y = a @ wt.T + b[:24]
    assert rel_l2(cpu_ops_clip.gemm_quickgelu_ref(a, wt, b[:24]), y * torch.sigmoid(1.702 * y)) <= 1e-6
    const = torch.full((2, 768), 300.0)
    out = cpu_ops_clip.layernorm_affine(const.to(BF), torch.ones(768), torch.full((768,), 0.3), torch.empty(2, 768, dtype=BF))
    assert torch.equal(out, torch.full((2, 768), 0.3).to(BF))
