"""TEST INFRASTRUCTURE ONLY -- f64 references, derived per-element tolerances and a torch emulation of the hand-scheduled
flash-attention kernels (attention_asm{72,72w,72p8,128,128p8,128q8}.hip + attn_merge_kernel).

The reference is taken over THE OPERANDS THE MFMA SEES, so that what remains between it and a kernel is the kernel's own arithmetic:
  Q   prescaled calls: the bf16 q as stored (log2 units).  Plain calls: load_q_bf16's fold restated, bf16(f32(q) * sc) with
      sc = f32(scale) * f32(log2 e) -- one extra bf16 rounding that the reference takes over, so no LSE slack is kept for it.
      qk8: the per-(row, head) e4m3 quantisation of include/osk.h (the rule restated in tests/test_gpu_attention_qk8.py).
  K   bf16 as stored; qk8: e4m3(clamp(K / s_k)) * s_k, one scale per (key batch, head).
  V   bf16 as stored; pv8 / qk8: the kernel's e4m3 V, from tests/cpu_ops.py::v_transpose_fp8 and v_scale_fp8's rule.

Tolerances (derived, not fitted).  With P_i the kernel's rounded probabilities, p_i the exact ones and P_i = p_i (1 + d_i),
    out_j - ref_j = sum_i p_i d_i (v_ij - ref_j) / sum_i p_i (1 + d_i)
because the denominator is the ones row of the SAME product and carries the same rounded P.

bf16 P: tools/gen_attn_asm.py converts P with v_cvt_pk_bf16_f32, which rounds to NEAREST even: |d_i| <= EPS = 2^-9 (not the 2^-8
of a truncation).  With dev_j = sum_i p_i |v_ij - ref_j|:
    tol_j  = C * EPS * dev_j + 2^-8 |ref_j| + FLOOR_BF16,      C = 2 (v_exp_f32 and the f32 score sums)
    |dlse| <= C * EPS + hd * 2^-24 * (1 + max_i |s_i|) * ln 2  (the f32 accumulation of a score over hd products)
e4m3 P (pv8, qk8): the running reference M stays within 2^8 of the row maximum ("fp8 mode"), so in reference units the
largest P of a row is at least 1; e4m3 has a relative error of 2^-4 on normal values and an absolute one of 2^-10 below 2^-6:
    e_i = max(2^-4 p_i, 2^-10 p_max),   tol_j = sum_i e_i |v_ij - ref_j| / (1 - sum_i e_i) + 2^-8 |ref_j| + FLOOR_FP8
    |dlse| <= ln(1 + 2^-4) + the f32 term
FLOORS: 0.  The floor is the smallest value the emulation below needs over every case of the table (tests/test_attention_refs.py),
  and it needs none: the f32 accumulation of P.V and the single bf16 rounding of the output stay under 2^-8 |ref_j| + the dev term
  even in the zero query row (every P the same power of two, d_i = 0) and in a one-key call (dev_j = 0, out = v exactly).
No further margin is given to a kernel.
"""
from __future__ import annotations

import math

import torch

from tests import cpu_ops

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
EPS_BF16 = 2.0 ** -9       # v_cvt_pk_bf16_f32: round to nearest even
C_BF16 = 2.0
FLOOR_BF16 = 0.0
FLOOR_FP8 = 0.0
E4M3_REL = 2.0 ** -4
E4M3_ABS = 2.0 ** -10
LSE_FP8 = math.log1p(2.0 ** -4)


def kernel_sc(scale: float) -> torch.Tensor:
    """the f32 factor attn_params() stores: scale * 1.4426950408889634f, an f32 product"""
    return torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)


def heads(t: torch.Tensor, H: int, hd: int) -> torch.Tensor:
    """[B, L, H*hd] -> [B, H, L, hd]"""
    B, L, _ = t.shape
    return t.reshape(B, L, H, hd).permute(0, 2, 1, 3)


def mfma_q(q: torch.Tensor, H: int, hd: int, scale: float, prescaled: bool, kind: str) -> torch.Tensor:
    """q bf16 [B, Lq, H*hd] -> the Q operand of the QK^T product in log2 units, f32 [B, H, Lq, hd]"""
    qf = heads(q.float(), H, hd)
    sc = torch.tensor(1.0) if prescaled else kernel_sc(scale)
    if kind == "qk8":
        qf = qf * sc
        amax = qf.abs().amax(-1, keepdim=True)
        sq = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
        return (qf / sq).clamp(-448, 448).to(F8).float() * sq
    return qf if prescaled else (qf * sc).to(BF).float()


def fp8_scales(x: torch.Tensor, H: int, hd: int) -> torch.Tensor:
    """x bf16 [n_seg, Bkv, seg, H*hd] -> f32 [Bkv, H]: absmax over every segment / 448 (1.0 for an all-zero head)"""
    n_seg, Bkv, seg, _ = x.shape
    amax = x.float().abs().reshape(n_seg, Bkv, seg, H, hd).amax(dim=(0, 2, 4))
    return torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)).contiguous()


def mfma_k(k: torch.Tensor, H: int, hd: int, kind: str, k_scale=None) -> torch.Tensor:
    """k bf16 [n_seg, Bkv, seg, H*hd] -> f32 [Bkv, H, n_seg*seg, hd] (segment s holds keys s*seg ..)"""
    n_seg, Bkv, seg, _ = k.shape
    kf = k.float().permute(1, 0, 2, 3).reshape(Bkv, n_seg * seg, H, hd).permute(0, 2, 1, 3)
    if kind == "qk8":
        s = k_scale[:, :, None, None]
        kf = (kf / s).clamp(-448, 448).to(F8).float() * s
    return kf


def mfma_v(v: torch.Tensor, H: int, hd: int, kind: str, v_scale=None) -> torch.Tensor:
    """v bf16 [n_seg, Bkv, seg, H*hd] -> f32 [Bkv, H, n_seg*seg, hd]: the bf16 V, or the e4m3 V the kernel multiplies"""
    n_seg, Bkv, seg, _ = v.shape
    if kind == "bf16":
        return v.float().permute(1, 0, 2, 3).reshape(Bkv, n_seg * seg, H, hd).permute(0, 2, 1, 3)
    segp = (seg + 63) // 64 * 64
    parts = []
    for s_ in range(n_seg):
        vt8 = torch.zeros(Bkv, H, cpu_ops.vt8_rows(hd), segp, dtype=torch.uint8)
        cpu_ops.v_transpose_fp8(v[s_], v_scale, vt8, H, hd)
        parts.append(vt8.view(F8).float()[:, :, :hd, :seg].permute(0, 1, 3, 2) * v_scale[:, :, None, None])   # [Bkv, H, seg, hd]
    return torch.cat(parts, 2)


def reference(qm, km, vm, kind: str, hd_sum: int | None = None):
    """f64 attention on MFMA operands: qm f32 [B, H, Lq, hd] (log2 units), km / vm f32 [Bkv, H, Lk, hd]; query batch b reads key
    batch b % Bkv.  Returns dict(out [B, H, Lq, hd], lse [B, H, Lq] (natural log), p [B, H, Lq, Lk], tol, lse_tol), all f64."""
    B, H, Lq, hd = qm.shape
    Bkv = km.shape[0]
    idx = torch.arange(B) % Bkv
    k, v = km.double()[idx], vm.double()[idx]
    s = qm.double() @ k.transpose(-1, -2)
    m = s.amax(-1, keepdim=True)
    e = torch.exp2(s - m)
    z = e.sum(-1, keepdim=True)
    p = e / z
    out = p @ v
    lse = (m + torch.log2(z)).squeeze(-1) * LN2
    if kind == "bf16":
        w = p * (C_BF16 * EPS_BF16)
        denom = torch.ones_like(z)
        floor, lse0 = FLOOR_BF16, C_BF16 * EPS_BF16
    else:
        w = torch.maximum(p * E4M3_REL, p.amax(-1, keepdim=True) * E4M3_ABS)
        denom = 1.0 - w.sum(-1, keepdim=True)
        assert (denom > 0).all(), "too many keys for the e4m3 bound to say anything"
        floor, lse0 = FLOOR_FP8, LSE_FP8
    dev = torch.empty_like(out)
    for b in range(B):                      # sum_i w_i |v_ij - ref_j| without a [Lq, Lk, hd] tensor per call
        for h in range(H):
            for r0 in range(0, Lq, 64):
                d = (v[b, h][None, :, :] - out[b, h, r0:r0 + 64][:, None, :]).abs()
                dev[b, h, r0:r0 + 64] = (w[b, h, r0:r0 + 64][:, :, None] * d).sum(1)
    tol = dev / denom + 2.0 ** -8 * out.abs() + floor
    lse_tol = lse0 + (hd_sum or hd) * 2.0 ** -24 * (1.0 + s.abs().amax(-1)) * LN2
    return dict(out=out, lse=lse, p=p, tol=tol, lse_tol=lse_tol, s=s)


# ---------------------------------------------------------------------------------------------------------------- emulation
def key_parts(n_seg: int, seg: int, split: int):
    """key index ranges of the parts of a split tail unit: key_part() of csrc/attention_params.h restated.  Whole segments per part
    when there are several, else runs of 64-key tiles of the one segment (only the last part ends in the ragged tile)."""
    if split == 1:
        return [(0, n_seg * seg)]
    if n_seg > 1:
        per = n_seg // split
        return [(p * per * seg, (p + 1) * per * seg) for p in range(split)]
    tps = (seg + 63) // 64
    return [(p * tps // split * 64, min((p + 1) * tps // split * 64, seg)) for p in range(split)]


def emulate(qm, km, vm, kind: str, m_mode, parts=None, merge_parts=None, mask=None, extra_den=()):
    """a kernel in torch on the CPU: scores in f32; P = 2^(s - M) rounded to bf16 (nearest even) or e4m3; the P.V product and the
    ones row accumulated in f32; one bf16 rounding of the output.  m_mode: "max" (M = the row maximum), "max-8" (the other end of
    the range the running reference is allowed), or a float (the FAST body: M = the bound).  parts: key ranges of a split tail unit
    (each part has its own M; partial O normalised in f32, log2-domain LSE) combined as attn_merge_kernel does; merge_parts: how
    many of them the merge sums, mask: f32 [Lk] key validity applied to the rounded P (what the ones row and V^T's zero padding do),
    extra_den: keys whose P enters the denominator once more -- the three mutants of tests/test_attention_refs.py.  Returns (out f32 [B, H, Lq, hd] holding bf16 values, lse f32 [B, H, Lq])."""
    B = qm.shape[0]
    idx = torch.arange(B) % km.shape[0]
    k, v = km.float()[idx], vm.float()[idx]
    s = qm.float() @ k.transpose(-1, -2)
    parts = parts or [(0, k.shape[2])]
    os_, ls_ = [], []
    for a, b_ in parts:
        sp = s[..., a:b_]
        if isinstance(m_mode, str):
            m = sp.amax(-1, keepdim=True) - (8.0 if m_mode == "max-8" else 0.0)
        else:
            m = torch.full_like(sp[..., :1], float(m_mode))
        pf = torch.exp2(sp - m)
        pr = pf.to(BF).float() if kind == "bf16" else pf.to(F8).float()
        if mask is not None:
            pr = pr * mask[a:b_]
        den = pr.sum(-1, keepdim=True)
        for i in extra_den:
            if a <= i < b_:
                den = den + pr[..., i - a:i - a + 1]
        os_.append((pr @ v[..., a:b_, :]) / den)
        ls_.append(m + torch.log2(den))
    if len(parts) == 1:
        return os_[0].to(BF).float(), ls_[0].squeeze(-1) * LN2
    n = len(parts) if merge_parts is None else merge_parts
    l = torch.stack(ls_[:n], 0)
    mm = l.amax(0)
    wgt = torch.exp2(l - mm)
    tot = wgt.sum(0)
    acc = sum(wgt[i] * os_[i] for i in range(n))
    return (acc / tot).to(BF).float(), (mm + torch.log2(tot)).squeeze(-1) * LN2


def ratios(out, lse, ref):
    """largest err / tol and dlse / tol of a result against a reference() dict; out [B, H, Lq, hd], lse [B, H, Lq]"""
    r_out = ((out.double() - ref["out"]).abs() / ref["tol"]).max().item()
    r_lse = ((lse.double() - ref["lse"]).abs() / ref["lse_tol"]).max().item()
    return r_out, r_lse
