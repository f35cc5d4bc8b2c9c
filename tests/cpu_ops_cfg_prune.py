"""TEST INFRASTRUCTURE ONLY -- tests/cpu_ops.py plus the CPU statement of the branch-count CFG combine (include/osk.h,
osk_cfg_euler_nb_bf16), with the call signature of open_sora_amd/_C.py, and its plain f64 reference.  A kernel table for
mmdit.set_ops_for_testing(): the not-gpu suite runs the sampler's pruned loop (I2VDenoiser.denoise(cfg_prune=True)) through it.
Never imported by the product path."""
from __future__ import annotations

import torch

from tests.cpu_ops import *          # noqa: F401,F403 -- the table is this module's namespace
from tests import cpu_ops as _base

F64 = torch.float64
CALLS = []     # (entry, ...) of every copy_rows / cfg_euler / cfg_euler_nb call: the tests read which path a loop took


def copy_rows(src, dst):
    CALLS.append(("copy_rows", dst.shape[0]))
    return _base.copy_rows(src, dst)


def cfg_euler(pred, x, x_out, g_txt, g_img, dt, g_img_vec=None):
    CALLS.append(("cfg_euler",))
    return _base.cfg_euler(pred, x, x_out, g_txt, g_img, dt, g_img_vec)


def cfg_euler_nb(pred, nb, x, x_out, g_txt, g_img, dt, g_img_vec=None):
    """f32 math in the kernel's operation order, one rounding; reads pred[:nb] only"""
    n = x.numel()
    _base._abi_check("osk_cfg_euler_nb_bf16", nb in (1, 2, 3), n > 0, n % 8 == 0, pred.numel() >= nb * n)
    CALLS.append(("cfg_euler_nb", nb))
    p = pred.reshape(-1)[: nb * n].float().reshape(nb, n)
    if nb == 3:
        gi = g_img if g_img_vec is None else g_img_vec.reshape(-1)
        v = p[2] + gi * (p[1] - p[2]) + g_txt * (p[0] - p[1])
    elif nb == 2:
        v = p[1] + g_txt * (p[0] - p[1])
    else:
        v = p[0]
    x_out.copy_((x.float().reshape(-1) + dt * v).reshape(x.shape).to(x_out.dtype))
    return x_out


def cfg_euler_nb_f64(pred: torch.Tensor, nb: int, x: torch.Tensor, g_txt: float, g_img, dt: float) -> torch.Tensor:
    """pred bf16 [>= nb, n] (cond, uncond, uncond_2), x bf16 [n], g_img a float or f32 [n] -> bf16-rounded f64 [n]:
    x + dt v with v = u2 + g_img (u - u2) + g_txt (c - u) | u + g_txt (c - u) | c for nb = 3 | 2 | 1; rows >= nb are not touched.
    g_txt, g_img and dt reach the kernel as f32."""
    f32 = lambda s: float(torch.tensor(s, dtype=torch.float32))
    p = pred[:nb].to(F64)
    if nb == 3:
        gi = g_img.to(F64) if torch.is_tensor(g_img) else f32(g_img)
        v = p[2] + gi * (p[1] - p[2]) + f32(g_txt) * (p[0] - p[1])
    elif nb == 2:
        v = p[1] + f32(g_txt) * (p[0] - p[1])
    else:
        v = p[0]
    return (x.to(F64) + f32(dt) * v).to(torch.float32).to(torch.bfloat16).to(F64)
