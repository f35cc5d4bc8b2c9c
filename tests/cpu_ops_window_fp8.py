"""TEST INFRASTRUCTURE ONLY -- tests/cpu_ops_window.py plus the CPU statement of the fp8 frame-window entry (include/osk.h,
osk_attention_fwd_window_fp8_bf16) and the qk8 preparation entries of tests/cpu_ops_sp_qk8.py, with the call signatures of
open_sora_amd/_C.py: a kernel table for mmdit.set_ops_for_testing() on which an fp8 model runs with the window on.  Beside it, what
the tests of that entry share: operands, the f64 reference over exactly each query block's key set on THE E4M3 OPERANDS THE KERNEL
MULTIPLIES, its derived tolerance, and a torch emulation of the two launches and the merge.  Never imported by the product path.

Tolerance (derived, not fitted): the formula of tests/cpu_ops_window.py with the e4m3 terms of tests/cpu_ops_attn_f64.py.
n_prefix == 0: launch A alone, cpu_ops_attn_f64.reference(kind) on the block's keys.  n_prefix > 0, with O_A the window-only and O_B
the prefix-only f64 output and w_A + w_B = 1 the f64 merge weights:
    tol     = w_A tol_A + w_B tol_B + 2^-9 w_A |O_A| + 2^-8 |ref|
    lse_tol = w_A lse_tol_A + w_B lse_tol_B + 2^-21 (1 + |lse|)
where tol_A, tol_B are reference(kind)["tol"] of each launch's own key set -- e_i = max(2^-4 p_i, 2^-10 p_max) per key, divided by
1 - sum_i e_i -- and lse_tol_A, lse_tol_B its ["lse_tol"] = ln(1 + 2^-4) + the f32 score term.  Each launch has its own running
reference, so each launch's p_max is its own: the terms are per launch, not those of one softmax over the union.
Condition on shapes: reference(kind) needs 1 - sum_i e_i > 0, and the absolute term grows as Lk 2^-10, so every query block's key
set, prefix included, stays at or below 576 keys: the denominator is then >= 1 - 2^-4 - 576 2^-10 = 0.375 for any operands."""
from __future__ import annotations

import torch

from tests.cpu_ops_window import *          # noqa: F401,F403 -- the table is this module's namespace
from tests import cpu_ops as _base
from tests import cpu_ops_attn_f64 as R
from tests import cpu_ops_window as _W
from tests.cpu_ops_sp_qk8 import attention_fwd_qk8, k8_shape, k_pack_fp8, kv_scale_fp8    # noqa: F401 -- entries cpu_ops lacks

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
KINDS = ("pv8", "qk8")
MAX_KEYS = 576
WINDOW_FP8_CALLS = []     # (n_prefix, mode, table as a tuple of rows, hd) of every call: the tests read which path a forward took


def _launch(qm, km, vm, m_mode="max"):
    """one launch of a pv8 / qk8 kernel on MFMA operands (f32 [.., Lq, hd], [.., Lk, hd]): scores in f32, P = 2^(s - M) rounded to
    e4m3, the denominator the sum of the SAME rounded P, O normalised in f32.  Returns (O f32, lse natural log [.., Lq])."""
    s = qm @ km.transpose(-1, -2)
    m = s.amax(-1, keepdim=True) - (8.0 if m_mode == "max-8" else 0.0)
    p = torch.exp2(s - m).to(F8).float()
    den = p.sum(-1, keepdim=True)
    return (p @ vm) / den, ((m + torch.log2(den)) * R.LN2).squeeze(-1)


def _two_launches(qm, km, vm, n_prefix, Lk, windows, m_mode="max", drop_prefix=False):
    """the entry as the kernels compute it, on MFMA operands qm [B, H, Lq, hd], km / vm [Bkv, H, Lk, hd]: per query block launch A
    over its window into bf16 rows and an f32 lse, launch B over the prefix into an f32 partial, the merge in f32 with one rounding
    (osk_attention_merge_into_bf16's rule).  drop_prefix: the merge never happens (a mutant).  Returns (out f32 [B, H, Lq, hd]
    holding bf16 values, lse f32 [B, H, Lq])."""
    idx = torch.arange(qm.shape[0]) % km.shape[0]
    km, vm = km.float()[idx], vm.float()[idx]
    Lq = qm.shape[2]
    outs, lses = [], []
    for i, (first, n) in enumerate(windows.tolist()):
        rows = slice(256 * i, min(256 * (i + 1), Lq))
        keys = _W.block_keys(n_prefix, Lk, first, n)[n_prefix:]
        oa, la = _launch(qm[:, :, rows].float(), km[:, :, keys], vm[:, :, keys], m_mode)
        oa = oa.to(BF).float()
        if n_prefix and not drop_prefix:
            ob, lb = _launch(qm[:, :, rows].float(), km[:, :, :n_prefix], vm[:, :, :n_prefix], m_mode)
            mm = torch.maximum(la, lb)
            ea, eb = torch.exp(la - mm), torch.exp(lb - mm)
            tot = ea + eb
            oa = ((ea / tot)[..., None] * oa + (eb / tot)[..., None] * ob).to(BF).float()
            la = mm + torch.log(tot)
        outs.append(oa)
        lses.append(la)
    return torch.cat(outs, 2), torch.cat(lses, 2)


def attention_fwd_window_fp8(q, k, k_scale, vt8, v_scale, out, H, hd, scale, *, n_prefix, windows, mode, lse=None, q_prescaled=False,
                             kv_batches=0, workspace=None, Lk=None):
    """CPU statement of osk_attention_fwd_window_fp8_bf16: K as given (mode "pv8": the bf16 view; "qk8": the packed bytes times
    k_scale, Q quantised per (row, head) as the kernel's prologue does), V from the e4m3 V^T times v_scale, then launch A per query
    block over its window, launch B over the prefix, the merge."""
    Bq, Lq, D = q.shape
    B = kv_batches if kv_batches else Bq
    RP = _base.vt8_rows(hd)
    if mode == "qk8":
        _base._abi_check("osk_attention_fwd_window_fp8_bf16 (qk8)", hd == 128, k.dtype == torch.uint8, Lk is not None,
                         tuple(k.shape) == k8_shape(B, H, Lk or 1), _base._al(k, 16), k_scale is not None and k_scale.numel() == B * H)
    else:
        _base._abi_check("osk_attention_fwd_window_fp8_bf16 (pv8)", mode == "pv8", hd in (72, 128), k.dtype == BF, k.stride(0) % 8 == 0,
                         k.stride(1) % 8 == 0, _base._al(k, 16))
        Lk = k.shape[1]
    Lp = (Lk + 63) // 64 * 64
    nqb, tiles = (Lq + 255) // 256, (Lk - n_prefix + 63) // 64
    _base._abi_check("osk_attention_fwd_window_fp8_bf16", q.stride(0) % 8 == 0, q.stride(1) % 8 == 0, _base._al(q, 16), _base._al(vt8, 16),
                     0 <= kv_batches <= Bq, n_prefix % 64 == 0, 0 <= n_prefix < Lk, tuple(windows.shape) == (nqb, 2),
                     windows.dtype == torch.int32, vt8.dtype == torch.uint8, tuple(vt8.shape) == (B, H, RP, Lp), v_scale.numel() == B * H,
                     n_prefix == 0 or (workspace is not None and out.stride(0) % 8 == 0 and out.stride(1) % 8 == 0 and _base._al(out, 16)))
    if bool((windows[:, 0] < 0).any()) or bool((windows[:, 1] < 1).any()) or bool((windows[:, 0] + windows[:, 1] > tiles).any()):
        raise ValueError("windows: a range outside the body's tiles")
    WINDOW_FP8_CALLS.append((n_prefix, mode, tuple(map(tuple, windows.tolist())), hd))
    f = vt8.view(F8).float()
    assert bool((f[:, :, hd, :Lk] == 1.0).all()) and bool((f[:, :, hd, Lk:] == 0.0).all()), "the validity row is not that of Lk keys"
    vm = f[:, :, :hd, :Lk].permute(0, 1, 3, 2) * v_scale.reshape(B, H, 1, 1)                   # [B, H, Lk, hd]
    qf = q.float().reshape(Bq, Lq, H, hd).permute(0, 2, 1, 3) * (1.0 if q_prescaled else scale * 1.4426950408889634)
    if mode == "qk8":
        km = k.view(F8).float()[:, :, :Lk] * k_scale.reshape(B, H, 1, 1)
        amax = qf.abs().amax(-1, keepdim=True)
        s_q = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
        qm = (qf / s_q).clamp(-448.0, 448.0).to(F8).float() * s_q
    else:
        km = k.float().reshape(B, Lk, H, hd).permute(0, 2, 1, 3)
        qm = qf if q_prescaled else qf.to(BF).float()
    o, l = _two_launches(qm, km, vm, n_prefix, Lk, windows)
    out.copy_(o.permute(0, 2, 1, 3).reshape(Bq, Lq, D).to(out.dtype))
    if lse is not None:
        lse.copy_(l)
    return out


# ---------------------------------------------------------------------------------------------------------------- test operands
def operands_fp8(hd: int, H: int, B: int, Bkv: int, Lq: int, Lk: int, seed: int = 0, bound: float = 48.0):
    """cpu_ops_window.operands with a query count of its own (the entry allows Lq != Lk): q (prescaled, log2 units) bf16
    [B, Lq, H*hd], k, v bf16 [Bkv, Lk, H*hd]; scores with a standard deviation of several log2 units -- a row's mass sits on a few
    keys, so a window that moves by a tile, or a prefix that goes missing, moves the output by far more than e4m3 noise."""
    g = torch.Generator().manual_seed(1000 * hd + 10 * Lk + Bkv + seed)
    k = torch.randn(Bkv, Lk, H * hd, generator=g).to(BF)
    v = torch.randn(Bkv, Lk, H * hd, generator=g).to(BF)
    q = torch.randn(B, Lq, H * hd, generator=g)
    kn = k.float().reshape(Bkv, Lk, H, hd).norm(dim=-1).max()
    qn = q.reshape(B, Lq, H, hd).norm(dim=-1).max()
    return (q * (bound / 1.02 / float(qn * kn))).to(BF), k, v


def mfma_operands(q, k, v, H: int, hd: int, kind: str):
    """(qm, km, vm, k_scale | None, v_scale): the operands the kernel of `kind` multiplies (tests/cpu_ops_attn_f64.py)"""
    ks = R.fp8_scales(k[None], H, hd) if kind == "qk8" else None
    vs = R.fp8_scales(v[None], H, hd)
    return R.mfma_q(q, H, hd, 1.0, True, kind), R.mfma_k(k[None], H, hd, kind, ks), R.mfma_v(v[None], H, hd, kind, vs), ks, vs


def reference(q, k, v, H: int, hd: int, n_prefix: int, windows: torch.Tensor, kind: str):    # noqa: F811 -- the fp8 kinds' version
    """cpu_ops_window.reference with the operands and the tolerance terms of an fp8 kind: f64 per query block over exactly that
    block's keys.  Returns dict(out [B, H, Lq, hd], lse [B, H, Lq], tol, lse_tol) in f64."""
    assert kind in KINDS, kind
    qm, km, vm, _, _ = mfma_operands(q, k, v, H, hd, kind)
    Lq, Lk = q.shape[1], k.shape[1]
    outs = {n_: [] for n_ in ("out", "lse", "tol", "lse_tol")}
    for i, (first, n) in enumerate(windows.tolist()):
        rows = slice(256 * i, min(256 * (i + 1), Lq))
        keys = _W.block_keys(n_prefix, Lk, first, n)
        assert len(keys) <= MAX_KEYS, (len(keys), "the e4m3 tolerance says nothing beyond this many keys (module docstring)")
        full = R.reference(qm[:, :, rows], km[:, :, keys], vm[:, :, keys], kind)
        if n_prefix == 0:
            tol, lse_tol = full["tol"], full["lse_tol"]
        else:
            a = R.reference(qm[:, :, rows], km[:, :, keys[n_prefix:]], vm[:, :, keys[n_prefix:]], kind)
            b = R.reference(qm[:, :, rows], km[:, :, :n_prefix], vm[:, :, :n_prefix], kind)
            wa, wb = torch.exp(a["lse"] - full["lse"])[..., None], torch.exp(b["lse"] - full["lse"])[..., None]
            assert torch.allclose(wa * a["out"] + wb * b["out"], full["out"], atol=1e-9)
            tol = wa * a["tol"] + wb * b["tol"] + 2.0 ** -9 * wa * a["out"].abs() + 2.0 ** -8 * full["out"].abs()
            lse_tol = wa[..., 0] * a["lse_tol"] + wb[..., 0] * b["lse_tol"] + 2.0 ** -21 * (1.0 + full["lse"].abs())
        for n_, t in (("out", full["out"]), ("lse", full["lse"]), ("tol", tol), ("lse_tol", lse_tol)):
            outs[n_].append(t)
    return {n_: torch.cat(ts, 2) for n_, ts in outs.items()}


def emulate(q, k, v, H: int, hd: int, n_prefix: int, windows: torch.Tensor, kind: str, m_mode="max", drop_prefix: bool = False):    # noqa: F811
    """cpu_ops_window.emulate for an fp8 kind: the two launches and the merge on the e4m3 operands, P rounded to e4m3"""
    qm, km, vm, _, _ = mfma_operands(q, k, v, H, hd, kind)
    return _two_launches(qm, km, vm, n_prefix, k.shape[1], windows, m_mode, drop_prefix)


# ---------------------------------------------------------------------------------------------------------------- the shared cases
H_, B_, NP, LQ = 2, 2, 64, 800                    # four query blocks, the last of 32 rows
BODIES = (448, 484)                               # seven full tiles; seven plus a 36-key ragged tile
FRAME = {448: 64, 484: 44}                        # frame sizes that divide the body (7 and 11 frames)
TABLES = ("w0", "w1", "hand", "hand_rev")
KIND_HD = (("pv8", 72), ("pv8", 128), ("qk8", 128))


def make_table(name: str, n_prefix: int, body: int) -> torch.Tensor:
    """four rows (LQ = 800).  w0 / w1: the rows of mmdit.attention_window_table for the joint sequence of n_prefix + body tokens
    (2 or 3 rows: the entry's Lq is not tied to Lk here), repeated in order until there are four.  hand: a 1-tile interior run, a
    2-tile run ending in the last tile, a run ending before the last tile, the last tile alone; hand_rev: the same rows in reverse
    order, so the 32-row last block meets the other end of the list."""
    from open_sora_amd.mmdit import attention_window_table

    tiles, nqb = (body + 63) // 64, (LQ + 255) // 256
    if name.startswith("hand"):
        rows = [(3, 1), (tiles - 2, 2), (1, tiles - 3), (tiles - 1, 1)]
        return torch.tensor(rows[::-1] if name == "hand_rev" else rows, dtype=torch.int32)
    t = attention_window_table(n_prefix, body, FRAME[body], int(name[1:]))
    return t[torch.arange(nqb) % t.shape[0]].contiguous()


_CASES: dict = {}


def case(kind: str, hd: int, body: int, Bkv: int, table: str, n_prefix: int = NP):
    """(q, k, v, table, reference) of one case, computed once per process and shared by the tests: treat it as read-only"""
    key = (kind, hd, body, Bkv, table, n_prefix)
    if key not in _CASES:
        q, k, v = operands_fp8(hd, H_, B_, Bkv, LQ, n_prefix + body)
        t = make_table(table, n_prefix, body)
        _CASES[key] = (q, k, v, t, reference(q, k, v, H_, hd, n_prefix, t, kind))
    return _CASES[key]
