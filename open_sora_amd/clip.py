"""MI355X-native CLIP text encoder (the reference's `HFEmbedder` CLIP branch, opensora/models/text/conditioner.py:9-53: Hugging
Face's `CLIPTextModel` for CLIP ViT-L/14 over 77 tokens, `attention_mask=None`, `pooler_output`) behind the Hugging Face state-dict
keys.

    ClipTextConfig / ClipTextModel   transformers' CLIPTextConfig / CLIPTextModel (quick_gelu text towers)
    ClipEmbedder                     conditioner.py:31-53 (tokenizer call, seq_align padding, `pooler_output`)

The nn.Modules only HOLD parameters.  All arithmetic except the embedding (a torch index of the token table plus the first L rows of
the position table: one add) and the pooling (a torch index) runs in the gfx950 kernels of include/osk.h through the kernel table
(mmdit.ops()); there is no eager fallback.  Exactly seven launches per layer:
    layer_norm1                      osk_layernorm_affine_bf16 (weight and bias, mean subtracted)
    q | k | v                        ONE osk_gemm_bf16 against the three weights and biases concatenated at plan time
    causal softmax(q k^T / 8) v      osk_attention_causal_bf16, q / k / v read in place from the fused projection output
    out_proj + residual              osk_gemm_bf16 with the bias and the res / gate epilogue (a gate of ones), in place on the hidden state
    layer_norm2                      osk_layernorm_affine_bf16
    quick_gelu(fc1 x)                osk_gemm_quickgelu_bf16
    fc2 + residual                   osk_gemm_bf16 with the bias and the res / gate epilogue
and one final LayerNorm over all rows: 7 * num_hidden_layers + 1 launches per forward (85 for CLIP-L).  The forward is bound by that
count, not by FLOPs.

The plan (kernel-side images of the weights: the fused q|k|v matrix and bias, f32 norm weights and biases) is built at the first
forward and dropped by `invalidate_plan()` / `load_state_dict`; it costs a second copy of the q, k and v weights.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
from torch import Tensor, nn

from . import mmdit as _m  # shares the kernel table (set_ops_for_testing) with the denoiser

BF16 = torch.bfloat16


def _ops():
    return _m.ops()


@dataclass
class ClipTextConfig:
    """the fields of transformers' CLIPTextConfig a text model reads"""

    vocab_size: int = 49408
    hidden_size: int = 512
    intermediate_size: int = 2048
    num_hidden_layers: int = 12
    num_attention_heads: int = 8
    max_position_embeddings: int = 77
    layer_norm_eps: float = 1e-5
    eos_token_id: int = 2
    hidden_act: str = "quick_gelu"

    @classmethod
    def clip_vit_l_14(cls) -> "ClipTextConfig":
        """openai/clip-vit-large-patch14, the reference's second text encoder (123 M text parameters)"""
        return cls(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                   max_position_embeddings=77, layer_norm_eps=1e-5, eos_token_id=2)


class ClipTextOutput(dict):
    """what ClipTextModel.forward returns: answers out["pooler_output"] (the reference indexes by key) and out.pooler_output"""

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
        raise RuntimeError(f"{type(self).__name__} holds parameters only; its arithmetic runs in libosk_hip.so (ClipTextModel.forward); "
                           "there is no eager fallback.")


class _Embeddings(_Holder):
    def __init__(self, cfg: ClipTextConfig):
        super().__init__()
        self.token_embedding = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.position_embedding = nn.Embedding(cfg.max_position_embeddings, cfg.hidden_size)


class _Attention(_Holder):
    def __init__(self, cfg: ClipTextConfig):
        super().__init__()
        d = cfg.hidden_size
        self.k_proj = nn.Linear(d, d)
        self.v_proj = nn.Linear(d, d)
        self.q_proj = nn.Linear(d, d)
        self.out_proj = nn.Linear(d, d)


class _MLP(_Holder):
    def __init__(self, cfg: ClipTextConfig):
        super().__init__()
        self.fc1 = nn.Linear(cfg.hidden_size, cfg.intermediate_size)
        self.fc2 = nn.Linear(cfg.intermediate_size, cfg.hidden_size)


class _Layer(_Holder):
    def __init__(self, cfg: ClipTextConfig):
        super().__init__()
        self.self_attn = _Attention(cfg)
        self.layer_norm1 = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)
        self.mlp = _MLP(cfg)
        self.layer_norm2 = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class _Encoder(_Holder):
    def __init__(self, cfg: ClipTextConfig):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(cfg) for _ in range(cfg.num_hidden_layers)])


class _Plan:
    """kernel-side images of the parameters"""

    def __init__(self, enc: "ClipTextModel"):
        def w(t):
            return t.detach().to(BF16).contiguous()

        def f32(t):
            return t.detach().float().contiguous()

        e = enc.embeddings
        dev = e.token_embedding.weight.device
        self.tok, self.pos = w(e.token_embedding.weight), w(e.position_embedding.weight)
        self.layers = []
        for ly in enc.encoder.layers:
            a, m = ly.self_attn, ly.mlp
            self.layers.append(dict(
                ln1=(f32(ly.layer_norm1.weight), f32(ly.layer_norm1.bias)),
                qkv=torch.cat([w(a.q_proj.weight), w(a.k_proj.weight), w(a.v_proj.weight)], 0),
                qkv_b=torch.cat([f32(a.q_proj.bias), f32(a.k_proj.bias), f32(a.v_proj.bias)], 0),
                o=w(a.out_proj.weight), o_b=f32(a.out_proj.bias),
                ln2=(f32(ly.layer_norm2.weight), f32(ly.layer_norm2.bias)),
                fc1=w(m.fc1.weight), fc1_b=f32(m.fc1.bias), fc2=w(m.fc2.weight), fc2_b=f32(m.fc2.bias)))
        self.final_ln = (f32(enc.final_layer_norm.weight), f32(enc.final_layer_norm.bias))
        self.ones_gate = torch.ones(1, enc.cfg.hidden_size, dtype=torch.float32, device=dev)
        self.buffers: dict = {}

    def workspace(self, cfg: ClipTextConfig, B: int, L: int):
        key = (B, L, id(_ops()))
        ws = self.buffers.get(key)
        if ws is None:
            dev, D = self.tok.device, cfg.hidden_size
            e = lambda *s: torch.empty(*s, dtype=BF16, device=dev)  # noqa: E731
            self.buffers.clear()
            ws = self.buffers[key] = dict(xn=e(B, L, D), qkv=e(B, L, 3 * D), att=e(B, L, D), ff=e(B, L, cfg.intermediate_size))
        return ws


class ClipTextModel(nn.Module):
    """transformers' CLIPTextModel for quick_gelu text towers, state-dict compatible with it (transformers 5 key names; a
    `text_model.` prefix -- transformers 4 and the published checkpoint -- is accepted on load)"""

    def __init__(self, cfg: ClipTextConfig):
        super().__init__()
        if cfg.hidden_act != "quick_gelu":
            raise ValueError(f"clip: hidden_act {cfg.hidden_act!r} is not built on the HIP path (osk_gemm_quickgelu_bf16 serves the "
                             "quick_gelu feed-forward of the OpenAI CLIP text towers)")
        if cfg.num_attention_heads < 1 or cfg.hidden_size != 64 * cfg.num_attention_heads:
            raise ValueError(f"clip: head dim {cfg.hidden_size / max(cfg.num_attention_heads, 1):g} (hidden_size {cfg.hidden_size} / "
                             f"{cfg.num_attention_heads} heads) is not built on the HIP path (osk_attention_causal_bf16 takes head dim 64)")
        if cfg.hidden_size % 64 or cfg.intermediate_size % 64:
            raise ValueError(f"clip: hidden_size {cfg.hidden_size} / intermediate_size {cfg.intermediate_size} must be multiples of 64 "
                             "(osk_gemm_bf16 takes K % 64 == 0)")
        if cfg.num_hidden_layers < 1:
            raise ValueError("clip: num_hidden_layers < 1")
        self.cfg = cfg
        self.embeddings = _Embeddings(cfg)
        self.encoder = _Encoder(cfg)
        self.final_layer_norm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)

    # ---- parameters
    @property
    def device(self):
        return self.embeddings.token_embedding.weight.device

    @property
    def dtype(self):
        return self.embeddings.token_embedding.weight.dtype

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
        """nn.Module.load_state_dict; keys under the `text_model.` prefix (transformers 4, the published checkpoint) lose it, and the
        `embeddings.position_ids` buffer older checkpoints store is ignored"""
        pre = "text_model."
        sd = {(k[len(pre):] if k.startswith(pre) else k): v for k, v in dict(state_dict).items()}
        sd.pop("embeddings.position_ids", None)
        self.invalidate_plan()
        return super().load_state_dict(sd, strict=strict, assign=assign)

    @classmethod
    def from_hf_module(cls, hf_clip) -> "ClipTextModel":
        """the plug-in for a reference user: `embedder.hf_module = ClipTextModel.from_hf_module(embedder.hf_module)`"""
        c = hf_clip.config
        c = getattr(c, "text_config", c)                    # a CLIPConfig carries the text tower's under text_config
        eos = c.eos_token_id
        cfg = ClipTextConfig(vocab_size=c.vocab_size, hidden_size=c.hidden_size, intermediate_size=c.intermediate_size,
                             num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads,
                             max_position_embeddings=c.max_position_embeddings, layer_norm_eps=c.layer_norm_eps,
                             eos_token_id=2 if eos is None else int(eos), hidden_act=getattr(c, "hidden_act", "quick_gelu"))
        sd = hf_clip.state_dict()
        w = next(iter(sd.values()))
        with torch.device(w.device):
            m = cls(cfg).to(w.dtype)
        m.load_state_dict(sd)
        return m.eval().requires_grad_(False)

    # ---- arithmetic
    @torch.no_grad()
    def forward(self, input_ids: Tensor, attention_mask=None, **ignored) -> ClipTextOutput:
        if attention_mask is not None:
            raise ValueError("clip: attention masks are not built on the HIP path; the reference calls its text encoder with "
                             "attention_mask=None (conditioner.py:48-52: pad tokens are attended, under the causal mask)")
        if input_ids.dim() != 2:
            raise ValueError(f"clip: input_ids must be [batch, tokens], got shape {tuple(input_ids.shape)}")
        cfg, ops, p = self.cfg, _ops(), self._plan()
        B, L = input_ids.shape
        if L > cfg.max_position_embeddings:
            raise ValueError(f"clip: {L} tokens exceed max_position_embeddings {cfg.max_position_embeddings}")
        H, D = cfg.num_attention_heads, cfg.hidden_size
        hd = D // H
        ws = p.workspace(cfg, B, L)
        xn, qkv, att, ff = ws["xn"], ws["qkv"], ws["att"], ws["ff"]
        ids = input_ids.to(p.tok.device)
        x = p.tok[ids] + p.pos[:L]                                 # [B, L, D] bf16, the residual stream (updated in place)
        rows = lambda t: t.view(1, B * L, t.shape[-1])            # noqa: E731  (the GEMMs see one batch of B * L rows)
        eps, scale = cfg.layer_norm_eps, hd ** -0.5
        for ly in p.layers:
            ops.layernorm_affine(x, *ly["ln1"], xn, eps)
            ops.gemm(rows(xn), ly["qkv"], ly["qkv_b"], rows(qkv))
            ops.attention_causal(qkv[:, :, :D], qkv[:, :, D: 2 * D], qkv[:, :, 2 * D:], att, H, hd, scale)
            ops.gemm(rows(att), ly["o"], ly["o_b"], rows(x), res=rows(x), gate=p.ones_gate)
            ops.layernorm_affine(x, *ly["ln2"], xn, eps)
            ops.gemm_quickgelu(rows(xn), ly["fc1"], ly["fc1_b"], rows(ff))
            ops.gemm(rows(ff), ly["fc2"], ly["fc2_b"], rows(x), res=rows(x), gate=p.ones_gate)
        out = ops.layernorm_affine(x, *p.final_ln, torch.empty_like(x), eps).to(self.dtype)
        # pooling as transformers does it: the checkpoints written with eos_token_id 2 take the row of the LARGEST id (the
        # end-of-text token has the highest id of CLIP's vocabulary), every other configuration the first eos_token_id
        if cfg.eos_token_id == 2:
            at = ids.argmax(dim=-1)
        else:
            at = (ids == cfg.eos_token_id).int().argmax(dim=-1)
        pooled = out[torch.arange(B, device=out.device), at]
        return ClipTextOutput(last_hidden_state=out, pooler_output=pooled)


# what the reference's text embedder asks of its tokenizer (conditioner.py:32-40): every prompt cut or padded to max_length
_TOKENIZER_OPTIONS = dict(truncation=True, return_length=False, return_overflowing_tokens=False, padding="max_length",
                          return_tensors="pt")


class ClipEmbedder(nn.Module):
    """prompts -> CLIP pooled vectors with the call signature of the CLIP branch of the reference's HFEmbedder (conditioner.py:9-53):
    `embedder(text, added_tokens=0, seq_align=1)`.  The tokenizer is passed in: this package loads none.  `hf_module`,
    `output_key` and `is_clip` are the attribute names the reference's callers read."""

    def __init__(self, tokenizer, encoder: nn.Module, max_length: int):
        super().__init__()
        self.tokenizer, self.max_length = tokenizer, max_length
        self.hf_module = encoder
        self.hf_module.eval()
        self.hf_module.requires_grad_(False)
        self.output_key, self.is_clip = "pooler_output", True

    def forward(self, text: list, added_tokens: int = 0, seq_align: int = 1) -> Tensor:
        ids = self.tokenizer(text, max_length=self.max_length, **_TOKENIZER_OPTIONS)["input_ids"]
        # the reference pads (added_tokens + tokens) up to a multiple of seq_align with pad tokens, for either encoder
        pad = -(added_tokens + ids.shape[1]) % seq_align
        if pad:
            ids = torch.cat([ids, ids.new_full((ids.shape[0], pad), self.tokenizer.pad_token_id)], dim=1)
        hidden = self.hf_module(input_ids=ids.to(self.hf_module.device), attention_mask=None, output_hidden_states=False)
        return hidden[self.output_key]
