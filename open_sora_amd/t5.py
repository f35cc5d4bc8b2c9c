"""MI355X-native T5 text encoder (the reference's `HFEmbedder` T5 branch, opensora/models/text/conditioner.py:9-53: Hugging Face's
`T5EncoderModel` for T5-v1.1-XXL over 512 tokens, `attention_mask=None`) behind the Hugging Face state-dict keys.

    T5EncoderConfig / T5Encoder      transformers' T5Config / T5EncoderModel (gated-gelu encoders: T5 v1.1)
    T5Embedder                       conditioner.py:31-53 (tokenizer call, seq_align padding, `last_hidden_state`)

The nn.Modules only HOLD parameters.  All arithmetic except the embedding lookup (a torch index) runs in the gfx950 kernels of
include/osk.h through the kernel table (mmdit.ops()); there is no eager fallback.  Per layer:
    T5LayerNorm                      osk_rmsnorm_affine_bf16 (weight, zero bias, no mean subtraction)
    q | k | v                        ONE osk_gemm_bf16 against the three weights concatenated at plan time
    softmax(q k^T + bias) v          osk_attention_relbias_bf16, q / k / v read in place from the fused projection output
    o + residual                     osk_gemm_bf16 with the res / gate epilogue (a gate of ones), in place on the hidden state
    T5LayerNorm                      osk_rmsnorm_affine_bf16
    gelu_new(wi_0 x) * (wi_1 x)      osk_gemm_geglu_bf16 (wi_0 = gate, wi_1 = value; its tanh GELU is gelu_new)
    wo + residual                    osk_gemm_bf16 with the res / gate epilogue
and one final T5LayerNorm.  The relative-position bias never exists as an [L, L] matrix: the bucket embedding of block 0 is
expanded once per sequence length into a [heads, 2 L - 1] f32 table indexed by the distance j - i.

The plan (kernel-side images of the weights: the fused q|k|v matrix, the packed GEGLU matrix, f32 norm weights) is built at the
first forward and dropped by `invalidate_plan()` / `load_state_dict`; it costs a second copy of the q, k, v, wi_0 and wi_1 weights.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
from torch import Tensor, nn

from . import mmdit as _m  # shares the kernel table (set_ops_for_testing) with the denoiser

BF16 = torch.bfloat16


def _ops():
    return _m.ops()


@dataclass
class T5EncoderConfig:
    """the fields of transformers' T5Config an encoder reads"""

    vocab_size: int = 32128
    d_model: int = 512
    d_kv: int = 64
    d_ff: int = 1024
    num_layers: int = 8
    num_heads: int = 6
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    layer_norm_epsilon: float = 1e-6

    @classmethod
    def t5_v1_1_xxl(cls) -> "T5EncoderConfig":
        """google/t5-v1_1-xxl, the reference's text encoder (4.7 G encoder parameters)"""
        return cls(vocab_size=32128, d_model=4096, d_kv=64, d_ff=10240, num_layers=24, num_heads=64)


def relative_position_bucket(relative_position: Tensor, num_buckets: int = 32, max_distance: int = 128) -> Tensor:
    """T5's BIDIRECTIONAL bucket of a relative position (key position - query position), from its definition (Raffel et al. 2020,
    section 2.1; mesh-tensorflow's `_relative_position_bucket`): half of the buckets per sign; per sign, distances below
    num_buckets / 4 each have their own bucket, larger ones share logarithmically wider buckets up to max_distance, and everything
    beyond falls into the last one.  The logarithm is evaluated in f32, as the implementations that trained the checkpoints do:
    the bucket edges are part of the model."""
    half = num_buckets // 2
    n = relative_position.abs()
    max_exact = half // 2
    log_ratio = torch.log(n.float() / max_exact) / math.log(max_distance / max_exact)
    large = (max_exact + (log_ratio * (half - max_exact)).to(torch.long)).clamp(max=half - 1)
    return (relative_position > 0).to(torch.long) * half + torch.where(n < max_exact, n, large)


class T5EncoderOutput(dict):
    """what T5Encoder.forward returns: answers out["last_hidden_state"] (the reference indexes by key) and out.last_hidden_state"""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


# =============================================================================================
# parameter containers (names == Hugging Face state-dict keys)
# =============================================================================================
class _Holder(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover - guard
        raise RuntimeError(f"{type(self).__name__} holds parameters only; its arithmetic runs in libosk_hip.so (T5Encoder.forward); "
                           "there is no eager fallback.")


class _LayerNorm(_Holder):
    def __init__(self, d: int):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))


class _Attention(_Holder):
    def __init__(self, cfg: T5EncoderConfig, has_relative_attention_bias: bool):
        super().__init__()
        inner = cfg.num_heads * cfg.d_kv
        self.q = nn.Linear(cfg.d_model, inner, bias=False)
        self.k = nn.Linear(cfg.d_model, inner, bias=False)
        self.v = nn.Linear(cfg.d_model, inner, bias=False)
        self.o = nn.Linear(inner, cfg.d_model, bias=False)
        if has_relative_attention_bias:
            self.relative_attention_bias = nn.Embedding(cfg.relative_attention_num_buckets, cfg.num_heads)


class _LayerSelfAttention(_Holder):
    def __init__(self, cfg: T5EncoderConfig, has_relative_attention_bias: bool):
        super().__init__()
        self.SelfAttention = _Attention(cfg, has_relative_attention_bias)
        self.layer_norm = _LayerNorm(cfg.d_model)


class _DenseGatedActDense(_Holder):
    def __init__(self, cfg: T5EncoderConfig):
        super().__init__()
        self.wi_0 = nn.Linear(cfg.d_model, cfg.d_ff, bias=False)
        self.wi_1 = nn.Linear(cfg.d_model, cfg.d_ff, bias=False)
        self.wo = nn.Linear(cfg.d_ff, cfg.d_model, bias=False)


class _LayerFF(_Holder):
    def __init__(self, cfg: T5EncoderConfig):
        super().__init__()
        self.DenseReluDense = _DenseGatedActDense(cfg)
        self.layer_norm = _LayerNorm(cfg.d_model)


class _Block(_Holder):
    def __init__(self, cfg: T5EncoderConfig, has_relative_attention_bias: bool):
        super().__init__()
        self.layer = nn.ModuleList([_LayerSelfAttention(cfg, has_relative_attention_bias), _LayerFF(cfg)])


class _Stack(_Holder):
    def __init__(self, cfg: T5EncoderConfig, embed_tokens: nn.Embedding):
        super().__init__()
        self.embed_tokens = embed_tokens
        self.block = nn.ModuleList([_Block(cfg, i == 0) for i in range(cfg.num_layers)])
        self.final_layer_norm = _LayerNorm(cfg.d_model)


class _Plan:
    """kernel-side images of the parameters"""

    def __init__(self, enc: "T5Encoder"):
        def w(t):
            return t.detach().to(BF16).contiguous()

        def f32(t):
            return t.detach().float().contiguous()

        dev = enc.shared.weight.device
        cfg = enc.cfg
        self.emb = w(enc.shared.weight)
        self.layers = []
        for blk in enc.encoder.block:
            at, ff = blk.layer[0], blk.layer[1]
            a, d = at.SelfAttention, ff.DenseReluDense
            wi, _ = _ops().geglu_pack(w(d.wi_1.weight), w(d.wi_0.weight))          # value = wi_1, gate = wi_0
            self.layers.append(dict(ln1=f32(at.layer_norm.weight), qkv=torch.cat([w(a.q.weight), w(a.k.weight), w(a.v.weight)], 0),
                                    o=w(a.o.weight), ln2=f32(ff.layer_norm.weight), wi=wi, wo=w(d.wo.weight)))
        self.final_ln = f32(enc.encoder.final_layer_norm.weight)
        self.zero_bias = torch.zeros(cfg.d_model, dtype=torch.float32, device=dev)
        self.ones_gate = torch.ones(1, cfg.d_model, dtype=torch.float32, device=dev)
        self.rel_emb = f32(enc.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight)   # [buckets, H]
        self.tables: dict = {}
        self.buffers: dict = {}

    def table(self, cfg: T5EncoderConfig, L: int) -> Tensor:
        """[H, 2 L - 1] f32: entry (h, d + L - 1) = the bias of head h between a query and the key d positions after it"""
        t = self.tables.get(L)
        if t is None:
            rel = torch.arange(-(L - 1), L, device=self.rel_emb.device)
            buckets = relative_position_bucket(rel, cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance)
            t = self.tables[L] = torch.empty(self.rel_emb.shape[1], 2 * L - 1, dtype=torch.float32, device=rel.device)
            t.copy_(self.rel_emb[buckets].t())
        return t

    def workspace(self, cfg: T5EncoderConfig, B: int, L: int):
        key = (B, L, id(_ops()))
        ws = self.buffers.get(key)
        if ws is None:
            dev, inner = self.emb.device, cfg.num_heads * cfg.d_kv
            e = lambda *s: torch.empty(*s, dtype=BF16, device=dev)  # noqa: E731
            self.buffers.clear()
            ws = self.buffers[key] = dict(xn=e(B, L, cfg.d_model), qkv=e(B, L, 3 * inner), att=e(B, L, inner), ff=e(B, L, cfg.d_ff),
                                          geglu=e(B * L, 2 * cfg.d_ff))
        return ws


class T5Encoder(nn.Module):
    """transformers' T5EncoderModel for gated-gelu (v1.1) encoders, state-dict compatible with it"""

    def __init__(self, cfg: T5EncoderConfig):
        super().__init__()
        if cfg.d_kv != 64:
            raise ValueError(f"t5: d_kv {cfg.d_kv} is not built on the HIP path (osk_attention_relbias_bf16 takes head dim 64)")
        if cfg.d_model % 64 or cfg.d_ff % 64:
            raise ValueError(f"t5: d_model {cfg.d_model} / d_ff {cfg.d_ff} must be multiples of 64 (osk_gemm_bf16 takes K % 64 == 0)")
        if cfg.num_layers < 1:
            raise ValueError("t5: num_layers < 1")
        self.cfg = cfg
        self.shared = nn.Embedding(cfg.vocab_size, cfg.d_model)
        self.encoder = _Stack(cfg, self.shared)             # encoder.embed_tokens IS shared (tied, as in transformers)

    # ---- parameters
    @property
    def device(self):
        return self.shared.weight.device

    @property
    def dtype(self):
        return self.shared.weight.dtype

    def invalidate_plan(self):
        self.__dict__.pop("_osk_plan", None)

    def _plan(self) -> _Plan:
        """cached; keyed on every parameter's (storage pointer, in-place version), so an in-place update rebuilds it"""
        key = tuple((q.data_ptr(), 0 if q.is_inference() else q._version) for q in self.parameters()) + (id(_ops()),)
        c = self.__dict__.get("_osk_plan")
        if c is None or c[0] != key:
            c = self.__dict__["_osk_plan"] = (key, _Plan(self))
        return c[1]

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """nn.Module.load_state_dict; a checkpoint that stores only one of the two tied embedding keys (safetensors files drop the
        duplicate) is completed with the other"""
        sd = dict(state_dict)
        a, b = "shared.weight", "encoder.embed_tokens.weight"
        if a in sd and b not in sd:
            sd[b] = sd[a]
        elif b in sd and a not in sd:
            sd[a] = sd[b]
        self.invalidate_plan()
        return super().load_state_dict(sd, strict=strict, assign=assign)

    @classmethod
    def from_hf_module(cls, hf_t5) -> "T5Encoder":
        """the plug-in for a reference user: `embedder.hf_module = T5Encoder.from_hf_module(embedder.hf_module)`"""
        c = hf_t5.config
        act = getattr(c, "feed_forward_proj", "gated-gelu")
        if act != "gated-gelu" or getattr(c, "dense_act_fn", "gelu_new") != "gelu_new":
            raise ValueError(f"t5: feed_forward_proj {act!r} is not built on the HIP path (osk_gemm_geglu_bf16 serves the gated "
                             "gelu_new feed-forward of T5 v1.1)")
        cfg = T5EncoderConfig(vocab_size=c.vocab_size, d_model=c.d_model, d_kv=c.d_kv, d_ff=c.d_ff, num_layers=c.num_layers,
                              num_heads=c.num_heads, relative_attention_num_buckets=c.relative_attention_num_buckets,
                              relative_attention_max_distance=c.relative_attention_max_distance,
                              layer_norm_epsilon=c.layer_norm_epsilon)
        w = hf_t5.shared.weight
        with torch.device(w.device):
            m = cls(cfg).to(w.dtype)
        m.load_state_dict(hf_t5.state_dict())
        return m.eval().requires_grad_(False)

    # ---- arithmetic
    @torch.no_grad()
    def forward(self, input_ids: Tensor, attention_mask=None, **ignored) -> T5EncoderOutput:
        if attention_mask is not None:
            raise ValueError("t5: attention masks are not built on the HIP path; the reference calls its text encoder with "
                             "attention_mask=None (conditioner.py:48-52: pad tokens are attended)")
        if input_ids.dim() != 2:
            raise ValueError(f"t5: input_ids must be [batch, tokens], got shape {tuple(input_ids.shape)}")
        cfg, ops, p = self.cfg, _ops(), self._plan()
        B, L = input_ids.shape
        H, hd, D = cfg.num_heads, cfg.d_kv, cfg.d_model
        inner = H * hd
        ws, table = p.workspace(cfg, B, L), p.table(cfg, L)
        xn, qkv, att, ff = ws["xn"], ws["qkv"], ws["att"], ws["ff"]
        x = p.emb[input_ids.to(p.emb.device)]                      # [B, L, D] bf16, the residual stream (updated in place)
        rows = lambda t: t.view(1, B * L, t.shape[-1])            # noqa: E731  (the GEMMs see one batch of B * L rows)
        eps = cfg.layer_norm_epsilon
        for ly in p.layers:
            ops.rmsnorm_affine(x, ly["ln1"], p.zero_bias, xn, eps)
            ops.gemm(rows(xn), ly["qkv"], None, rows(qkv))
            ops.attention_relbias(qkv[:, :, :inner], qkv[:, :, inner: 2 * inner], qkv[:, :, 2 * inner:], att, H, hd, 1.0, table)
            ops.gemm(rows(att), ly["o"], None, rows(x), res=rows(x), gate=p.ones_gate)
            ops.rmsnorm_affine(x, ly["ln2"], p.zero_bias, xn, eps)
            ops.gemm_geglu(rows(xn), ly["wi"], None, rows(ff), workspace=ws["geglu"])
            ops.gemm(rows(ff), ly["wo"], None, rows(x), res=rows(x), gate=p.ones_gate)
        out = ops.rmsnorm_affine(x, p.final_ln, p.zero_bias, torch.empty_like(x), eps)
        return T5EncoderOutput(last_hidden_state=out.to(self.dtype))


# what the reference's text embedder asks of its tokenizer (conditioner.py:32-40): every prompt cut or padded to max_length
_TOKENIZER_OPTIONS = dict(truncation=True, return_length=False, return_overflowing_tokens=False, padding="max_length",
                          return_tensors="pt")


class T5Embedder(nn.Module):
    """prompts -> T5 hidden states with the call signature of the T5 branch of the reference's HFEmbedder (conditioner.py:9-53):
    `embedder(text, added_tokens=0, seq_align=1)`.  The tokenizer is passed in: this package loads none.  `hf_module`,
    `output_key` and `is_clip` are the attribute names the reference's callers read."""

    def __init__(self, tokenizer, encoder: nn.Module, max_length: int):
        super().__init__()
        self.tokenizer, self.max_length = tokenizer, max_length
        self.hf_module = encoder
        self.hf_module.eval()
        self.hf_module.requires_grad_(False)
        self.output_key, self.is_clip = "last_hidden_state", False

    def forward(self, text: list, added_tokens: int = 0, seq_align: int = 1) -> Tensor:
        ids = self.tokenizer(text, max_length=self.max_length, **_TOKENIZER_OPTIONS)["input_ids"]
        # the sequence-parallel denoiser wants (added_tokens + tokens) to divide by seq_align: pad tokens fill the gap
        pad = -(added_tokens + ids.shape[1]) % seq_align
        if pad:
            ids = torch.cat([ids, ids.new_full((ids.shape[0], pad), self.tokenizer.pad_token_id)], dim=1)
        hidden = self.hf_module(input_ids=ids.to(self.hf_module.device), attention_mask=None, output_hidden_states=False)
        return hidden[self.output_key]
