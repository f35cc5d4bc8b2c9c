"""LoRA adapters for the MI355X-native MMDiT, merged on the device when the plan is built.

Serves the `pretrained_lora_path` branch of the reference's prepare_api (opensora/utils/sampling.py:542-545:
`PeftModel.from_pretrained(model, path, is_trainable=False)`) for the adapters its trainer writes in peft's on-disk format
(scripts/diffusion/train.py:208-216, opensora/utils/ckpt.py:421-422).  peft is not needed and never imported: the adapter
directory is read directly (`json`, `safetensors` / `torch.load`).

How it works: nothing here computes a side path.  `load_lora` records, per adapted nn.Linear, the (A, B, scale) triples in a side
table of open_sora_amd/mmdit.py; the next plan build takes `bf16(W + sum_i scale_i B_i A_i)` (osk_lora_merge_bf16: f32 sums, one
rounding for ALL adapters of the Linear) instead of the zero-copy view of W.  Every GEMM, epilogue, pair / group launch and
attention kernel of the step then runs exactly as without adapters, at no cost per step; the price is one extra copy of each adapted
weight.  The parameters and `state_dict()` of the model are never touched, so unloading is exact.  fp8 mode quantises the merged
weight (adapters and `enable_fp8` compose in either order).

A hipGraph captured before `load_lora` / `set_lora_weights` / `unload_lora` replays the OLD weights' buffers, as after any plan
rebuild: capture again after changing adapters.

The on-disk layout handled here is written down from peft's documented format (adapter_config.json + adapter_model.safetensors with
`base_model.model.<module path>.lora_A.weight` [r, in] / `.lora_B.weight` [out, r]); it has not been checked against a peft
installation.
"""
from __future__ import annotations

import json
import math
import os
import re
from dataclasses import dataclass, field

import torch
from torch import Tensor, nn

from . import mmdit

BF16 = torch.bfloat16
MAX_RANK = 256          # osk_lora_merge_bf16
MAX_ADAPTERS = 8        # ... per Linear, in one call
_PREFIX = "base_model.model."
_BLOCKS = ("double_blocks.", "single_blocks.")


@dataclass
class LoraModule:
    """one adapted Linear: delta W = scale * B @ A"""
    a: Tensor          # lora_A.weight [r, in]
    b: Tensor          # lora_B.weight [out, r]
    r: int
    alpha: float
    scale: float       # alpha / r, or alpha / sqrt(r) with use_rslora


@dataclass
class LoraAdapter:
    """a peft LoRA adapter as read from disk (or built by hand): module path inside the MMDiT -> LoraModule"""
    modules: dict = field(default_factory=dict)
    config: dict = field(default_factory=dict)
    path: str | None = None


def _pattern_value(pattern: dict, module_path: str, default):
    """peft's rule for rank_pattern / alpha_pattern: the first key with `(.*\\.)?<key>$` matching the module path"""
    for key, val in (pattern or {}).items():
        if re.match(rf"(.*\.)?{key}$", module_path):
            return val
    return default


def _refuse(cfg: dict) -> None:
    if cfg.get("peft_type", "LORA") != "LORA":
        raise ValueError(f"peft_type = {cfg.get('peft_type')!r}: only LORA adapters can be merged")
    if cfg.get("use_dora"):
        raise ValueError("use_dora: DoRA rescales the merged weight per column, which this merge does not express")
    if cfg.get("bias", "none") != "none":
        raise ValueError(f"bias = {cfg.get('bias')!r}: adapters that train biases are not supported (bias must be 'none')")
    if cfg.get("fan_in_fan_out"):
        raise ValueError("fan_in_fan_out: the adapter stores transposed weights (Conv1D layers); the MMDiT has nn.Linear only")
    if cfg.get("modules_to_save"):
        raise ValueError(f"modules_to_save = {cfg.get('modules_to_save')!r}: fully trained copies of modules are not supported")


def _check_against(model: nn.Module, adapter: LoraAdapter) -> None:
    for path, m in adapter.modules.items():
        try:
            lin = model.get_submodule(path)
        except AttributeError:
            raise ValueError(f"adapter key {path!r}: the model has no such module") from None
        if not isinstance(lin, nn.Linear):
            raise ValueError(f"adapter key {path!r}: {type(lin).__name__} is not an nn.Linear")
        out_f, in_f = lin.weight.shape
        if tuple(m.a.shape) != (m.r, in_f) or tuple(m.b.shape) != (out_f, m.r):
            raise ValueError(f"adapter key {path!r}: lora_A {tuple(m.a.shape)} / lora_B {tuple(m.b.shape)} do not fit the Linear's "
                             f"weight shape {(out_f, in_f)} at rank {m.r}")


def read_peft_adapter(path: str, model: nn.Module | None = None) -> LoraAdapter:
    """Read a peft LoRA adapter directory: adapter_config.json + adapter_model.safetensors (or, when that file is absent,
    adapter_model.bin through torch.load(weights_only=True)).  ValueError, naming the field, for anything the merge cannot
    express: another peft_type, use_dora, bias != "none", fan_in_fan_out, modules_to_save, keys outside the Linear layers of
    double_blocks / single_blocks (the reference adapts only those: opensora/models/mmdit/model.py:198), inconsistent shapes --
    and, with `model` given (load_lora passes it), a key that names no nn.Linear of it or a shape that does not fit its Linear."""
    with open(os.path.join(path, "adapter_config.json")) as f:
        cfg = json.load(f)
    _refuse(cfg)
    st_path = os.path.join(path, "adapter_model.safetensors")
    if os.path.isfile(st_path):
        from safetensors.torch import load_file

        sd = load_file(st_path)
    else:
        sd = torch.load(os.path.join(path, "adapter_model.bin"), map_location="cpu", weights_only=True)
    halves: dict = {}
    for key, t in sd.items():
        k = key[len(_PREFIX):] if key.startswith(_PREFIX) else key
        m = re.fullmatch(r"(.+)\.lora_([AB])\.weight", k)
        if m is None:
            raise ValueError(f"adapter key {key!r}: not a `<module path>.lora_A.weight` / `.lora_B.weight` tensor")
        mod_path, which = m.group(1), m.group(2)
        if not mod_path.startswith(_BLOCKS):
            raise ValueError(f"adapter key {key!r}: only the Linear layers inside double_blocks / single_blocks can be adapted")
        if t.dim() != 2:
            raise ValueError(f"adapter key {key!r}: expected a 2-D weight, got shape {tuple(t.shape)}")
        halves.setdefault(mod_path, {})[which] = t
    r0, alpha0 = cfg.get("r", 8), cfg.get("lora_alpha", 8)
    rslora = bool(cfg.get("use_rslora", False))
    adapter = LoraAdapter(config=cfg, path=path)
    for mod_path, h in sorted(halves.items()):
        if set(h) != {"A", "B"}:
            raise ValueError(f"adapter key {mod_path!r}: lora_{'B' if 'A' in h else 'A'}.weight is missing")
        a, b = h["A"], h["B"]
        r = int(_pattern_value(cfg.get("rank_pattern"), mod_path, r0))
        alpha = float(_pattern_value(cfg.get("alpha_pattern"), mod_path, alpha0))
        if a.shape[0] != r or b.shape[1] != r:
            raise ValueError(f"adapter key {mod_path!r}: lora_A {tuple(a.shape)} / lora_B {tuple(b.shape)} do not have the rank r = {r} "
                             "that r / rank_pattern give this module")
        if not 1 <= r <= MAX_RANK:
            raise ValueError(f"adapter key {mod_path!r}: r = {r} outside 1 .. {MAX_RANK}")
        adapter.modules[mod_path] = LoraModule(a, b, r, alpha, alpha / math.sqrt(r) if rslora else alpha / r)
    if model is not None:
        _check_against(model, adapter)
    return adapter


# ----------------------------------------------------------------------------------------------
# adapters on a model
# ----------------------------------------------------------------------------------------------
@dataclass
class _Loaded:
    adapter: LoraAdapter
    weight: float
    dev: dict = field(default_factory=dict)     # module path -> (A bf16, B bf16) on the Linear's device


def _registry(model) -> dict:
    reg = model.__dict__.get("_osk_lora")
    if reg is None:
        reg = {}
        object.__setattr__(model, "_osk_lora", reg)   # (_osk_*: dropped by copy.deepcopy / pickle, like the plan -- a copy is the base model)
    return reg


def _blocks(model):
    return list(getattr(model, "double_blocks", ())) + list(getattr(model, "single_blocks", ()))


def _refresh(model) -> None:
    """rebuild the per-Linear side table from the registry, bump the epoch that is part of the plan keys, drop the plans"""
    reg = _registry(model)
    table: dict = {}
    for ld in reg.values():
        if ld.weight == 0.0:
            continue                                  # an adapter at weight 0 costs nothing: the Linear keeps its zero-copy view
        for path, m in ld.adapter.modules.items():
            a, b = ld.dev[path]
            table.setdefault(path, []).append((a, b, m.scale * ld.weight))
    for path, ads in table.items():
        if len(ads) > MAX_ADAPTERS:
            raise ValueError(f"{path}: {len(ads)} active adapters on one Linear, at most {MAX_ADAPTERS}")
    for b in _blocks(model):
        for m in b.modules():
            if isinstance(m, nn.Linear):
                mmdit._LORA.pop(m, None)
    for path, ads in table.items():
        mmdit._LORA[model.get_submodule(path)] = ads
    for m in [model] + _blocks(model):
        object.__setattr__(m, "_osk_lora_epoch", m.__dict__.get("_osk_lora_epoch", 0) + 1)
    if hasattr(model, "invalidate_plan"):
        model.invalidate_plan()
    else:
        for b in _blocks(model):
            if "_osk_plan" in b.__dict__:
                object.__delattr__(b, "_osk_plan")


def load_lora(model: nn.Module, path_or_adapter, name: str = "default", weight: float = 1.0) -> LoraAdapter:
    """Activate an adapter (a peft directory or a LoraAdapter) on the model under `name` at `weight` (a factor on its scale).
    Replaces `PeftModel.from_pretrained(model, path, is_trainable=False)`.  Several adapters may be active on one Linear: they
    reach the kernel in one call and the merged weight is rounded once.  Bumps the plan epoch and drops the plan: the next
    forward rebuilds it with merged copies of the adapted weights (a graph captured before is stale, see the module docstring)."""
    reg = _registry(model)
    if name in reg:
        raise ValueError(f"an adapter named {name!r} is already loaded: unload_lora(model, {name!r}) first")
    adapter = path_or_adapter if isinstance(path_or_adapter, LoraAdapter) else read_peft_adapter(os.fspath(path_or_adapter), model)
    _check_against(model, adapter)
    for path in adapter.modules:
        if not path.startswith(_BLOCKS):
            raise ValueError(f"adapter key {path!r}: only the Linear layers inside double_blocks / single_blocks can be adapted")
    ld = _Loaded(adapter, float(weight))
    for path, m in adapter.modules.items():
        dev = model.get_submodule(path).weight.device
        ld.dev[path] = (m.a.detach().to(device=dev, dtype=BF16).contiguous(), m.b.detach().to(device=dev, dtype=BF16).contiguous())
    reg[name] = ld
    try:
        _refresh(model)
    except ValueError:
        del reg[name]
        _refresh(model)
        raise
    return adapter


def set_lora_weights(model: nn.Module, weights: dict) -> None:
    """{name: weight}: change the factor on the scale of loaded adapters (0.0 switches one off without unloading it)."""
    reg = _registry(model)
    for name in weights:
        if name not in reg:
            raise KeyError(f"no adapter named {name!r} is loaded (loaded: {sorted(reg)})")
    for name, w in weights.items():
        reg[name].weight = float(w)
    _refresh(model)


def unload_lora(model: nn.Module, name: str | None = None) -> None:
    """Drop one adapter, or all of them (name None).  The base parameters were never modified: the model is exactly what it was."""
    reg = _registry(model)
    if name is None:
        reg.clear()
    elif name in reg:
        del reg[name]
    else:
        raise KeyError(f"no adapter named {name!r} is loaded (loaded: {sorted(reg)})")
    _refresh(model)


def lora_report(model: nn.Module) -> list:
    """per loaded adapter: its name, weight, source path and the modules it adapts with their rank and scale (weight not applied)"""
    return [{"name": name, "weight": ld.weight, "path": ld.adapter.path,
             "modules": {p: {"r": m.r, "scale": m.scale} for p, m in ld.adapter.modules.items()}}
            for name, ld in _registry(model).items()]


def merged_weight(model: nn.Module, module_path: str) -> Tensor:
    """the bf16 weight the plan uses for that Linear: W itself without active adapters, else bf16(W + sum_i scale_i B_i A_i)"""
    lin = model.get_submodule(module_path)
    if not isinstance(lin, nn.Linear):
        raise ValueError(f"{module_path!r} is not an nn.Linear")
    return mmdit._lin_w(lin)
