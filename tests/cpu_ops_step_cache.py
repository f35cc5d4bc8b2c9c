"""TEST INFRASTRUCTURE ONLY -- tests/cpu_ops.py (with the branch-count combine of tests/cpu_ops_cfg_prune.py) plus the CPU
statement of the sampler's step cache (include/osk.h: osk_step_delta_bf16, osk_residual_sub_bf16, osk_residual_add_bf16), with the call signatures of open_sora_amd/_C.py; their plain
f64 references; and the step-cached sampling loop stated on the oracle's fp32 forward.  A kernel table
for mmdit.set_ops_for_testing(): the not-gpu suite and the GPU tests' comparator run I2VDenoiser.denoise(step_cache=...) through
it.  Never imported by the product path."""
from __future__ import annotations

import math

import torch

from oracle import mmdit_oracle as O, sampling_oracle as S
from tests.cpu_ops_cfg_prune import *          # noqa: F401,F403 -- the table is this module's namespace (cpu_ops + cfg_euler_nb)
from tests import cpu_ops as _base

F64 = torch.float64
BF = torch.bfloat16
CALLS = []     # (entry, rows) of every step_delta / residual_sub / residual_add call: the tests read which path a step took


# ----------------------------------------------------------------------------- the kernel table's three entries
def _view_ok(t) -> bool:
    return (t.dtype == BF and t.ndim == 3 and t.numel() > 0 and t.shape[2] % 8 == 0 and t.stride(2) == 1 and t.stride(0) % 8 == 0
            and t.stride(1) % 8 == 0 and _base._al(t, 16))


def step_delta_workspace_bytes(B, L, C):
    chunks = B * L * (C // 8)
    return 8 * max(1, min(2048, (chunks + 255) // 256))


def step_delta(cur, prev, sums, workspace):
    """f32 sums (torch's own summation order: the kernel's is its own, both within the chain bound of the f64 statement)"""
    _base._abi_check("osk_step_delta_bf16", _view_ok(cur), _view_ok(prev), prev.is_contiguous(), prev.shape == cur.shape,
                     sums.dtype == torch.float32 and sums.numel() == 2, workspace.numel() >= step_delta_workspace_bytes(*cur.shape))
    CALLS.append(("step_delta", cur.shape[0]))
    c, p = cur.float(), prev.float()
    sums[0] = (c - p).abs().sum()
    sums[1] = p.abs().sum()
    prev.copy_(cur)
    return sums


def residual_sub(a, b, out):
    _base._abi_check("osk_residual_sub_bf16", _view_ok(a), _view_ok(b), _view_ok(out), a.shape == b.shape == out.shape)
    CALLS.append(("residual_sub", a.shape[0]))
    out.copy_((a.float() - b.float()).to(BF))
    return out


def residual_add(a, b, out):
    _base._abi_check("osk_residual_add_bf16", _view_ok(a), _view_ok(b), _view_ok(out), a.shape == b.shape == out.shape)
    CALLS.append(("residual_add", a.shape[0]))
    out.copy_((a.float() + b.float()).to(BF))
    return out


# ----------------------------------------------------------------------------- f64 statements of the kernels
def step_delta_f64(cur: torch.Tensor, prev: torch.Tensor) -> tuple[float, float]:
    """(sum |cur - prev|, sum |prev|) of two bf16 tensors in f64: no rounding that matters"""
    c, p = cur.to(F64), prev.to(F64)
    return float((c - p).abs().sum()), float(p.abs().sum())


def residual_f64(a: torch.Tensor, b: torch.Tensor, add: bool) -> torch.Tensor:
    """bf16(a +- b): the exact result (f64 holds the sum of two bf16 values whose exponents are < 45 apart exactly) rounded ONCE.
    f64 -> bf16 directly: a detour through f32 would round twice."""
    r = a.to(F64) + b.to(F64) if add else a.to(F64) - b.to(F64)
    return r.to(BF)


def distance(num: float, den: float) -> float:
    """d of DESIGN.md section 4 from the two sums"""
    if not (math.isfinite(num) and math.isfinite(den)) or den == 0.0:
        return math.inf
    return num / den


# ----------------------------------------------------------------------------- the rule on the oracle's forward
def i2v_denoise_step_cache(sd: dict, cfg: dict, img3: torch.Tensor, timesteps, guidance: float, guidance_img: float, masks, masked_ref,
                           counts, threshold: float, coefficients=None, text_osci=False, image_osci=False,
                           scale_temporal_osci=False, patch_size: int = 2, **model_kwargs):
    """oracle/sampling_oracle.py::i2v_denoise with the step cache stated on the oracle's forward, in img3.dtype (fp32: no rounding
    of M, R or Y), step i on the counts[i] leading branches with the branch-count combine of tests/cpu_ops_cfg_prune.py.  The
    decision is the product's own pure function.  Returns (x, [(d, acc, computed)])."""
    from open_sora_amd.sampling import step_cache_decide

    rope_mode = "half" if cfg.get("use_liger_rope", False) else "interleaved"
    n = img3.shape[0] // 3
    dt = img3.dtype
    b, c, t, d3, d4 = masked_ref.shape
    cond = S.pack(torch.cat((masks, masked_ref), 1), patch_size)
    cond3 = torch.cat([cond, cond, torch.zeros_like(cond)], 0)
    tripled = {k: v for k, v in model_kwargs.items() if torch.is_tensor(v) and v.shape[0] == 3 * n}
    x = img3[:n]
    n_steps = len(timesteps) - 1
    R = [None] * (3 * n)
    m_prev, acc, record = None, 0.0, []
    for i, (t_curr, t_prev) in enumerate(zip(timesteps[:-1], timesteps[1:])):
        nb = counts[i]
        m = nb * n
        kw = dict(model_kwargs, **{k: v[:m] for k, v in tripled.items()})
        X, txt, vec, ang = O.prepare_block_inputs(sd, cfg, torch.cat([x] * nb, 0), cond=cond3[:m], timesteps=torch.full((m,), t_curr, dtype=dt),
                                                  guidance=torch.full((m,), guidance, dtype=dt) if cfg.get("guidance_embed", False) else None,
                                                  **kw)
        sh1, sc1 = O._modulation(sd, "double_blocks.0.img_mod", vec, 6)[:2]
        M = ((1 + sc1) * O._layer_norm(X) + sh1)[:n]
        d = math.inf if m_prev is None else distance(*step_delta_f64(M, m_prev))
        m_prev = M
        computed, acc = step_cache_decide(i, n_steps, d, acc, threshold, coefficients, all(r is not None for r in R[:m]))
        if computed:
            img, tx = X, txt
            for j in range(cfg["depth"]):
                img, tx = O.double_block(sd, cfg, j, img, tx, vec, ang, rope_mode)
            y = torch.cat((tx, img), 1)
            for j in range(cfg["depth_single_blocks"]):
                y = O.single_block(sd, cfg, j, y, vec, ang, rope_mode)
            Y = y[:, tx.shape[1]:]
            for r in range(m):
                R[r] = Y[r] - X[r]
        else:
            Y = X + torch.stack(R[:m])
        pred = O.last_layer(sd, Y, vec)
        record.append((d, acc, computed))
        tg = S.oscillation_gs(guidance, i) if text_osci else guidance
        ig = S.oscillation_gs(guidance_img, i) if image_osci else guidance_img
        if nb == 3:
            pc, pu, pu2 = pred.chunk(3, 0)
            if ig > 1.0 and scale_temporal_osci:
                upper = torch.linspace(ig, 1.0, len(timesteps))[i]
                ramp = torch.linspace(1.0, float(upper), t)[None, None, :, None, None].repeat(b, c, 1, d4, d3)
                ig = S.pack(ramp, patch_size).to(dt)
            v = pu2 + ig * (pu - pu2) + tg * (pc - pu)
        elif nb == 2:
            pc, pu = pred.chunk(2, 0)
            v = pu + tg * (pc - pu)
        else:
            v = pred
        x = x + (t_prev - t_curr) * v
    return x, record
