"""CPU: host side of the T5 text encoder (open_sora_amd.t5), driven through the CPU emulation of the kernels' semantics
(tests/cpu_ops_t5.py), and the plain-torch restatement the GPU tests take as truth (tests/t5_restatement.py) pinned to the output
transformers itself produced (tests/golden/t5_small.npz, recorded by tools/make_golden_t5.py) and, where transformers imports, to the
live model.  The kernel itself is checked on the GPU by tests/test_gpu_t5.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import cpu_ops_t5
from tests import t5_restatement as R
from tests.util import assert_parity, finite_retry, rel_l2
from tools.make_golden_t5 import BIAS_LENGTHS, input_ids, small_state_dict

BF = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t5_small.npz")

HAVE_HF = importlib.util.find_spec("transformers") is not None
needs_hf = pytest.mark.skipif(not HAVE_HF, reason="needs transformers")


@pytest.fixture()
def emu(hip_lib):
    from open_sora_amd import mmdit, t5

    mmdit.set_ops_for_testing(cpu_ops_t5)
    yield t5
    mmdit.set_ops_for_testing(hip_lib)


@pytest.fixture(scope="module")
def golden():
    return {k: v for k, v in np.load(GOLDEN).items()}


def small_model(T, dtype=BF):
    m = T.T5Encoder(T.T5EncoderConfig(**R.SMALL)).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in small_state_dict().items()})
    return m


def restated(ids, dtype=torch.float32):
    sd = {k: v.to(dtype) for k, v in small_state_dict().items()}
    with torch.no_grad():
        return R.encode(sd, R.SMALL, ids)


# ------------------------------------------------------------------------------------------------ restatement == transformers
def test_restatement_matches_golden(golden):
    ids = torch.from_numpy(golden["input_ids"])
    assert torch.equal(ids, input_ids()), "the seeded generator no longer reproduces the recorded input_ids"
    out, want = restated(ids), torch.from_numpy(golden["last_hidden_state"])
    assert out.shape == want.shape == (2, 192, 256)
    assert rel_l2(out, want) <= 1e-5, rel_l2(out, want)            # fp32 round-off of 2 layers (sums in another order)


def test_restatement_bf16_is_a_fair_comparator(golden):
    """the restatement's bf16 run rounds where transformers' bf16 run rounds: the two are equally far from the fp32 output"""
    want = torch.from_numpy(golden["last_hidden_state"])
    hf16 = torch.from_numpy(golden["last_hidden_state_bf16_bits"]).view(BF)
    ours16 = finite_retry(lambda: restated(torch.from_numpy(golden["input_ids"]), BF))
    e_hf, e_re = rel_l2(hf16, want), rel_l2(ours16, want)
    assert 0.5 * e_hf <= e_re <= 2.0 * e_hf, (e_hf, e_re)


@needs_hf
def test_restatement_matches_live_transformers():
    from tools.make_golden_t5 import hf_last_hidden_state, hf_model

    sd = small_state_dict()
    m = hf_model(R.SMALL, sd)
    g = torch.Generator().manual_seed(5)
    for shape in ((1, 7), (2, 65), (1, 300)):
        ids = torch.randint(0, R.SMALL["vocab_size"], shape, generator=g)
        assert rel_l2(restated(ids), hf_last_hidden_state(m, ids)) <= 1e-5


# ----------------------------------------------------------------------------------------------- relative-distance table
@pytest.mark.parametrize("L", BIAS_LENGTHS)
def test_distance_table_equals_recorded_compute_bias(emu, golden, L):
    m = small_model(emu, torch.float32)
    table = m._plan().table(m.cfg, L)
    want = torch.from_numpy(golden[f"bias_{L}"])
    assert table.dtype == torch.float32 and tuple(table.shape) == (4, 2 * L - 1) and table.is_contiguous()
    assert torch.equal(table, want)
    assert m._plan().table(m.cfg, L) is table                       # cached per L
    # and the restatement's [H, L, L] matrix is that table, entry (j - i) + L - 1
    assert torch.equal(R.toeplitz_table(R.compute_bias(small_state_dict(), R.SMALL, L)), want)


def test_bucket_function_from_its_definition(emu):
    """half of the buckets per sign, exact below num_buckets / 4, logarithmic up to max_distance, the last bucket beyond"""
    rel = torch.arange(-600, 601)
    b = emu.relative_position_bucket(rel, 32, 128)
    assert torch.equal(b, R.relative_position_bucket(rel, 32, 128))
    at = lambda d: int(b[d + 600])  # noqa: E731
    assert [at(-d) for d in range(8)] == list(range(8)) and [at(d) for d in range(1, 8)] == [16 + d for d in range(1, 8)]
    assert at(-8) == 8 and at(8) == 24
    assert at(-90) == 14 and at(-91) == 15 and at(-128) == 15 and at(-600) == 15 and at(90) == 30 and at(128) == 31 and at(600) == 31   # 8 * 16^(7/8) = 90.5
    neg = b[:601].flip(0)
    assert bool((neg[1:] >= neg[:-1]).all()) and int(b.min()) == 0 and int(b.max()) == 31      # monotone in the distance
    assert torch.equal(b[601:], neg[1:] + 16)                       # the positive side mirrors the negative one


@needs_hf
@pytest.mark.parametrize("L", (1, 2, 65, 300))
def test_distance_table_matches_live_transformers(emu, L):
    from tools.make_golden_t5 import hf_bias_table, hf_model

    m = small_model(emu, torch.float32)
    assert torch.equal(m._plan().table(m.cfg, L), hf_bias_table(hf_model(R.SMALL, small_state_dict()), L))


# --------------------------------------------------------------------------------------------------------- state dict
def test_state_dict_keys_match_the_generator(emu, golden):
    want = [str(k) for k in golden["keys"]]
    m = small_model(emu)
    sd = m.state_dict()
    assert list(sd) == want == list(small_state_dict()) == list(R.param_shapes(R.SMALL))
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v) for k, v in R.param_shapes(R.SMALL).items()}
    assert m.encoder.embed_tokens.weight is m.shared.weight         # tied
    assert sum("relative_attention_bias" in k for k in want) == 1 and "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight" in want


def test_xxl_preset_keys_and_shapes(emu):
    cfg = emu.T5EncoderConfig.t5_v1_1_xxl()
    assert (cfg.vocab_size, cfg.d_model, cfg.d_kv, cfg.d_ff, cfg.num_layers, cfg.num_heads) == (32128, 4096, 64, 10240, 24, 64)
    assert (cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance, cfg.layer_norm_epsilon) == (32, 128, 1e-6)
    with torch.device("meta"):
        m = emu.T5Encoder(cfg)
    shapes = R.param_shapes(dict(vocab_size=32128, d_model=4096, d_kv=64, d_ff=10240, num_layers=24, num_heads=64,
                                 relative_attention_num_buckets=32))
    sd = m.state_dict()
    assert list(sd) == list(shapes) and {k: tuple(v.shape) for k, v in sd.items()} == shapes
    assert sum(p.numel() for p in m.parameters()) == 4_762_310_656


def test_load_state_dict_is_strict_and_completes_the_tied_key(emu):
    m = emu.T5Encoder(emu.T5EncoderConfig(**R.SMALL))
    sd = small_state_dict()
    m.load_state_dict(sd)
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    for tied in ("shared.weight", "encoder.embed_tokens.weight"):   # a safetensors file stores one of the two
        short = {k: v for k, v in sd.items() if k != tied}
        m2 = emu.T5Encoder(emu.T5EncoderConfig(**R.SMALL))
        m2.load_state_dict(short)
        assert torch.equal(m2.shared.weight, sd["shared.weight"])
    short = dict(sd)
    short.pop("encoder.block.1.layer.1.DenseReluDense.wi_1.weight")
    with pytest.raises(RuntimeError, match="wi_1"):
        m.load_state_dict(short)
    extra = dict(sd)
    extra["encoder.block.1.layer.0.SelfAttention.relative_attention_bias.weight"] = torch.zeros(32, 4)
    with pytest.raises(RuntimeError, match="block.1.layer.0.SelfAttention.relative_attention_bias"):
        m.load_state_dict(extra)


@needs_hf
def test_from_hf_module_round_trips(emu):
    from tools.make_golden_t5 import hf_model

    sd = small_state_dict()
    hf = hf_model(R.SMALL, sd, BF)
    m = emu.T5Encoder.from_hf_module(hf)
    assert m.cfg == emu.T5EncoderConfig(**R.SMALL) and m.dtype == BF and not m.training
    got, want = m.state_dict(), hf.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    hf.load_state_dict(got, strict=True)                            # and back
    ids = input_ids()[:, :40]
    out = m(input_ids=ids, attention_mask=None, output_hidden_states=False)
    assert_parity(out["last_hidden_state"], restated(ids), finite_retry(lambda: restated(ids, BF)), "from_hf_module forward")


@needs_hf
def test_from_hf_module_refuses_a_relu_feed_forward(emu):
    from tools.make_golden_t5 import _without_specless_modules

    with _without_specless_modules():
        from transformers import T5Config, T5EncoderModel

        hf = T5EncoderModel(T5Config(vocab_size=32, d_model=64, d_kv=64, d_ff=64, num_layers=1, num_heads=1, feed_forward_proj="relu"))
    with pytest.raises(ValueError, match="feed_forward_proj 'relu'"):
        emu.T5Encoder.from_hf_module(hf)


def test_unsupported_configurations_are_refused_at_construction(emu):
    for field, value, match in (("d_kv", 32, "d_kv 32"), ("d_model", 200, "d_model 200"), ("d_ff", 520, "d_ff 520"),
                                ("num_layers", 0, "num_layers")):
        cfg = dict(R.SMALL)
        cfg[field] = value
        with pytest.raises(ValueError, match=match):
            emu.T5Encoder(emu.T5EncoderConfig(**cfg))


# ------------------------------------------------------------------------------------- the encoder through the emulated kernels
def test_emulated_forward_matches_restatement_and_golden(emu, golden):
    ids = torch.from_numpy(golden["input_ids"])
    m = small_model(emu)
    out = m(input_ids=ids, attention_mask=None, output_hidden_states=False)
    assert out["last_hidden_state"] is out.last_hidden_state and list(out) == ["last_hidden_state"]
    y = out.last_hidden_state
    assert y.dtype == BF and tuple(y.shape) == (2, 192, 256)
    ref_bf16 = finite_retry(lambda: restated(ids, BF))
    assert_parity(y, restated(ids), ref_bf16, "emulated T5 encoder vs restatement")
    assert_parity(y, torch.from_numpy(golden["last_hidden_state"]), torch.from_numpy(golden["last_hidden_state_bf16_bits"]).view(BF),
                  "emulated T5 encoder vs transformers' recorded output")


@pytest.mark.parametrize("shape", [(1, 1), (3, 65), (1, 520)])
def test_emulated_forward_other_lengths(emu, shape):
    ids = torch.randint(0, R.SMALL["vocab_size"], shape, generator=torch.Generator().manual_seed(shape[1]))
    y = small_model(emu)(ids).last_hidden_state
    assert_parity(y, restated(ids), finite_retry(lambda: restated(ids, BF)), f"emulated T5 encoder {shape}")


def test_forward_runs_only_kernel_table_ops_in_the_documented_order(emu, monkeypatch):
    calls = []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(cpu_ops_t5, name)

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
        mmdit.set_ops_for_testing(cpu_ops_t5)
    layer = ["rmsnorm_affine", "gemm", "attention_relbias", "gemm", "rmsnorm_affine", "gemm_geglu", "gemm"]
    assert calls == ["geglu_pack"] * 2 + layer * 2 + ["rmsnorm_affine"]


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
    sd["encoder.final_layer_norm.weight"] = sd["encoder.final_layer_norm.weight"] * 2
    m.load_state_dict({k: v.to(BF) for k, v in sd.items()})
    y1 = m(ids).last_hidden_state
    assert rel_l2(y1, 2 * y0.float()) <= 2.0 ** -7                  # load_state_dict dropped the plan
    with torch.no_grad():
        m.encoder.final_layer_norm.weight.mul_(0.5)                 # an in-place update is seen through the version counter
    assert rel_l2(m(ids).last_hidden_state, y0) <= 2.0 ** -7
    p = m._plan()
    m.invalidate_plan()
    assert m._plan() is not p


# ------------------------------------------------------------------------------------------------------------- T5Embedder
class _StubTokenizer:
    pad_token_id = 0

    def __init__(self, n_tokens):
        self.n_tokens, self.calls = n_tokens, []

    def __call__(self, text, **kw):
        self.calls.append((list(text), kw))
        ids = torch.arange(1, self.n_tokens + 1).repeat(len(text), 1) % 100 + 1
        return {"input_ids": ids}


class _StubEncoder(torch.nn.Module):
    device = torch.device("cpu")

    def forward(self, input_ids, attention_mask="unset", **kw):
        self.seen = (input_ids.clone(), attention_mask, kw)
        return {"last_hidden_state": input_ids[..., None].float()}


@pytest.mark.parametrize("n_tokens,added,align,want", [(512, 0, 7, 518), (512, 0, 1, 512), (512, 0, 8, 512), (512, 4, 8, 516),
                                                       (512, 6, 7, 512), (300, 1, 64, 319)])
def test_embedder_reproduces_the_seq_align_padding(emu, n_tokens, added, align, want):
    tok, enc = _StubTokenizer(n_tokens), _StubEncoder()
    e = emu.T5Embedder(tok, enc, max_length=n_tokens)
    out = e(["a prompt", ""], added_tokens=added, seq_align=align)
    ids, mask, kw = enc.seen
    assert tuple(ids.shape) == (2, want) and (added + want) % align == 0 and tuple(out.shape) == (2, want, 1)
    assert torch.equal(ids[:, :n_tokens], tok(["a", "b"])["input_ids"]) and bool((ids[:, n_tokens:] == tok.pad_token_id).all())
    assert mask is None and kw == {"output_hidden_states": False}
    text, call = tok.calls[0]
    assert text == ["a prompt", ""]
    assert call == dict(truncation=True, max_length=n_tokens, return_length=False, return_overflowing_tokens=False,
                        padding="max_length", return_tensors="pt")
    assert e.output_key == "last_hidden_state" and e.hf_module is enc and not e.is_clip


def test_embedder_around_the_emulated_encoder(emu):
    m = small_model(emu)
    e = emu.T5Embedder(_StubTokenizer(20), m, max_length=20)
    y = e(["x"], seq_align=16)
    ids = torch.nn.functional.pad(_StubTokenizer(20)(["x"])["input_ids"], (0, 12), value=0)
    assert tuple(y.shape) == (1, 32, 256) and torch.equal(y, m(ids).last_hidden_state)


# ------------------------------------------------------------------------------------------------------- the emulation itself
def test_emulated_attention_matches_the_restatement():
    g = torch.Generator().manual_seed(2)
    B, L, H = 2, 70, 3
    q, k, v = (torch.randn(B, L, H * 64, generator=g) for _ in range(3))
    full = 5.0 * torch.randn(H, 2 * L + 3, generator=g)
    idx = torch.arange(L)[None, :] - torch.arange(L)[:, None] + L - 1
    want = R.attention(*(t.double().view(B, L, H, 64) for t in (q, k, v)), full.double()[:, idx]).reshape(B, L, H * 64)
    got = cpu_ops_t5.attention_relbias_ref(q, k, v, H, 64, 1.0, full, dtype=torch.float64)
    assert rel_l2(got, want) <= 1e-6                                # (the restatement's softmax is f32 whatever the operands are)
    want = R.attention(*(t.double().view(B, L, H, 64) for t in (q, k, v)), None, 0.125).reshape(B, L, H * 64)
    assert rel_l2(cpu_ops_t5.attention_relbias_ref(q, k, v, H, 64, 0.125, None, dtype=torch.float64), want) <= 1e-6


def test_emulated_geglu_matches_the_unpacked_formula():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(1, 300, 64, generator=g).to(BF)
    wv, wg = (torch.randn(48, 64, generator=g).to(BF) / 8 for _ in range(2))
    wp, _ = cpu_ops_t5.geglu_pack(wv, wg)
    assert tuple(wp.shape) == (96, 64) and torch.equal(wp[:16], wv[:16]) and torch.equal(wp[16:32], wg[:16])   # blocks of 16, value first
    with pytest.raises(RuntimeError, match="status -2"):               # a narrow N needs the workspace, as in the library
        cpu_ops_t5.gemm_geglu(a, wp, None, torch.empty(1, 300, 48, dtype=BF))
    out = cpu_ops_t5.gemm_geglu(a, wp, None, torch.empty(1, 300, 48, dtype=BF), workspace=torch.empty(300 * 96, dtype=BF))
    want = (a.float() @ wv.float().T) * torch.nn.functional.gelu(a.float() @ wg.float().T, approximate="tanh")
    assert rel_l2(out, want) <= 2.0 ** -8
