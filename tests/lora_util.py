"""Shared helpers of the LoRA tests: seeded adapters for a tiny MMDiT config, peft-format directories written with `json` and
`safetensors` only, and the fp32 state dict with W <- W + s B A (the truth the model-level tests compare against)."""
import json
import os

import torch

from oracle import synth


def linear_paths(cfg: dict) -> list:
    """every nn.Linear inside the double / single blocks (modulation layers included), by module path"""
    qkv = ["qkv"] if cfg["fused_qkv"] else ["q_proj", "k_proj", "v_proj"]
    out = []
    for i in range(cfg["depth"]):
        for s in ("img", "txt"):
            out += [f"double_blocks.{i}.{s}_attn.{q}" for q in qkv]
            out += [f"double_blocks.{i}.{s}_attn.proj", f"double_blocks.{i}.{s}_mlp.0", f"double_blocks.{i}.{s}_mlp.2",
                    f"double_blocks.{i}.{s}_mod.lin"]
    for i in range(cfg["depth_single_blocks"]):
        lin1 = ["linear1"] if cfg["fused_qkv"] else ["q_proj", "k_proj", "v_mlp"]
        out += [f"single_blocks.{i}.{n}" for n in lin1 + ["linear2", "modulation.lin"]]
    return out


def make_modules(cfg: dict, sd32: dict, seed: int, r: int, alpha: float, rel: float = 0.3, paths=None, rslora: bool = False) -> dict:
    """{module path: (A [r, in], B [out, r])} with bf16-representable f32 entries; B is sized so that the Frobenius norm of
    scale * B A is about `rel` times that of the Linear's weight (scale = alpha / r, or alpha / sqrt(r))"""
    shapes = synth.mmdit_param_shapes(cfg)
    g = torch.Generator().manual_seed(7919 * seed + 13)
    scale = alpha / (r ** 0.5 if rslora else r)
    mods = {}
    for p in (paths if paths is not None else linear_paths(cfg)):
        out_f, in_f = (int(s) for s in shapes[p + ".weight"])
        a = (torch.randn(r, in_f, generator=g) * in_f ** -0.5).bfloat16().float()
        b = torch.randn(out_f, r, generator=g)
        b = (b * (rel * float(sd32[p + ".weight"].float().norm()) / max(float((scale * (b @ a)).norm()), 1e-30))).bfloat16().float()
        mods[p] = (a, b)
    return mods


def write_peft_dir(path, mods: dict, r: int, alpha: float, fmt: str = "safetensors", **config) -> str:
    """an adapter directory in peft's on-disk format: adapter_config.json + adapter_model.safetensors (or .bin)"""
    from safetensors.torch import save_file

    path = os.fspath(path)
    os.makedirs(path, exist_ok=True)
    cfg = dict(peft_type="LORA", r=r, lora_alpha=alpha, bias="none", use_dora=False, use_rslora=False, fan_in_fan_out=False,
               modules_to_save=None, rank_pattern={}, alpha_pattern={}, target_modules=sorted({p.split(".")[-1] for p in mods}))
    cfg.update(config)
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(cfg, f)
    sd = {}
    for p, (a, b) in mods.items():
        sd[f"base_model.model.{p}.lora_A.weight"] = a.contiguous()
        sd[f"base_model.model.{p}.lora_B.weight"] = b.contiguous()
    if fmt == "safetensors":
        save_file(sd, os.path.join(path, "adapter_model.safetensors"))
    else:
        torch.save(sd, os.path.join(path, "adapter_model.bin"))
    return path


def merged_state_dict(sd32: dict, *adapters) -> dict:
    """fp32 state dict with W <- W + sum scale * B A; adapters = (mods, scale) pairs"""
    sd = dict(sd32)
    for mods, scale in adapters:
        for p, (a, b) in mods.items():
            sd[p + ".weight"] = sd[p + ".weight"] + scale * (b.double() @ a.double()).float()
    return sd
