"""TEST INFRASTRUCTURE ONLY -- tests/cpu_ops_window_fp8.py (and with it tests/cpu_ops_window.py) plus the CPU statement of the anchored
frame-window entry (include/osk.h, osk_attention_fwd_window_anchor_bf16), of the three-part in-place merge
(osk_attention_merge_into2_bf16) and the kv_join statement of tests/cpu_ops_sp_window.py, with the call signatures of
open_sora_amd/_C.py: a kernel table for mmdit.set_ops_for_testing() on which a bf16 or fp8 model runs with anchor frames, on one
device and with ranks as threads.  Beside it, what the tests of that entry share: the stated key set of a query block (prefix, run,
suffix), the f64 reference over exactly that set with its derived tolerance.  Never imported by the product path.

Tolerance (derived, not fitted): tests/cpu_ops_window.py's rule with one more partial.  out = w_A O_A + w_B O_B + w_C O_C with the f64
merge weights (sum 1), O_A the run-only, O_B the prefix-only, O_C the suffix-only output:
    tol     = w_A tol_A + w_B tol_B + w_C tol_C + 2^-9 w_A |O_A| + 2^-8 |ref|
    lse_tol = w_A lse_tol_A + w_B lse_tol_B + w_C lse_tol_C + 2^-20 (1 + |lse|)
the launches' own tolerances (tests/cpu_ops_attn_f64.reference of the operand kind on each launch's own key set -- each launch has
its own running maximum), launch A's bf16 rounding of its finished rows, ONE final rounding (the three-part merge rounds once; B and
C stay f32), and for the LSE the f32 exp / log / sum of the merge kernel -- one exp and one add more than the two-part merge's
2^-21, hence 2^-20.  A missing part (n_prefix == 0 or n_suffix == 0) drops its term; without either the tolerance is launch A's.
Condition on shapes in the fp8 kinds (tests/cpu_ops_window_fp8.py): every LAUNCH's key set stays at or below 576 keys."""
from __future__ import annotations

import threading

import torch

from tests.cpu_ops_window_fp8 import *          # noqa: F401,F403 -- the table is this module's namespace
from tests import cpu_ops as _base
from tests import cpu_ops_attn_f64 as R
from tests import cpu_ops_window_fp8 as _F
from tests.cpu_ops_sp_window import kv_join, CALLS as SP_CALLS    # noqa: F401 -- the join of a sharded windowed forward
from tests.cpu_ops_ragged import attention_fwd_ragged, attention_ragged_workspace    # noqa: F401

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
ANCHOR_CALLS: dict = {}   # thread ident -> [(mode, Lq, Lk, n_prefix, n_suffix, score_bound, table rows)] of every anchored call
_LOCK = threading.Lock()


def anchor_calls():
    """every recorded call, whichever thread made it"""
    with _LOCK:
        return [c for cs in ANCHOR_CALLS.values() for c in cs]


def attention_window_anchor_workspace_bytes(B, H, Lq, hd):
    return 16


def attention_window_anchor_workspace(B, H, Lq, hd, device):
    return torch.empty(16, dtype=torch.uint8, device=device)


def anchor_key_sets(n_prefix: int, n_suffix: int, Lk: int, first: int, n: int):
    """(prefix, run, suffix) key indices of a query block with table row (first, n): disjoint by construction of the entry"""
    s0 = Lk - n_suffix
    a, b = n_prefix + 64 * first, min(n_prefix + 64 * (first + n), s0)
    return torch.arange(n_prefix), torch.arange(a, b), torch.arange(s0, Lk)


def anchor_mask(Lq: int, Lk: int, n_prefix: int, n_suffix: int, windows: torch.Tensor) -> torch.Tensor:
    """bool [Lq, Lk]: the block-granular mask the entry states"""
    m = torch.zeros(Lq, Lk, dtype=torch.bool)
    for i, (first, n) in enumerate(windows.tolist()):
        m[256 * i: 256 * (i + 1), torch.cat(anchor_key_sets(n_prefix, n_suffix, Lk, first, n))] = True
    return m


def attention_fwd_window_anchor(q, k, vt, out, H, hd, scale, *, n_prefix, n_suffix, windows, mode="bf16", k_scale=None, v_scale=None,
                                lse=None, q_prescaled=False, kv_batches=0, score_bound=0.0, workspace=None, Lk=None):
    """CPU statement of osk_attention_fwd_window_anchor_bf16: the operands of the mode as tests/cpu_ops_window.py / cpu_ops_window_fp8.py
    read them, dense f32 scores with the block-granular three-part mask, one softmax, one rounding"""
    Bq, Lq, D = q.shape
    B = kv_batches if kv_batches else Bq
    if mode != "qk8":
        Lk = k.shape[1]
    Lp = (Lk + 63) // 64 * 64
    s0 = Lk - n_suffix
    nqb, tiles = (Lq + 255) // 256, (s0 - n_prefix + 63) // 64
    _base._abi_check("osk_attention_fwd_window_anchor_bf16", mode in ("bf16", "pv8", "qk8"), q.stride(0) % 8 == 0, q.stride(1) % 8 == 0,
                     _base._al(q, 16), _base._al(k, 16), _base._al(vt, 16), 0 <= kv_batches <= Bq, n_prefix % 64 == 0, 0 <= n_prefix < Lk,
                     n_suffix >= 0, n_suffix == 0 or (s0 % 64 == 0 and s0 > n_prefix), tuple(windows.shape) == (nqb, 2),
                     windows.dtype == torch.int32, score_bound >= 0,
                     workspace is not None and out.stride(0) % 8 == 0 and out.stride(1) % 8 == 0 and _base._al(out, 16))
    if bool((windows[:, 0] < 0).any()) or bool((windows[:, 1] < 1).any()) or bool((windows[:, 0] + windows[:, 1] > tiles).any()):
        raise ValueError("windows: a range outside the body's tiles")
    with _LOCK:
        ANCHOR_CALLS.setdefault(threading.get_ident(), []).append(
            (mode, Lq, Lk, n_prefix, n_suffix, float(score_bound), tuple(map(tuple, windows.tolist()))))
    qf = q.float().reshape(Bq, Lq, H, hd).permute(0, 2, 1, 3) * (1.0 if q_prescaled else scale * 1.4426950408889634)
    if mode == "bf16":
        key2pos = torch.empty(Lp, dtype=torch.long)
        key2pos[_base.pos2key(hd, Lp)] = torch.arange(Lp)
        km = k.float().reshape(B, Lk, H, hd).permute(0, 2, 1, 3)
        vm = vt.float().reshape(B, H, hd, Lp)[..., key2pos][..., :Lk].permute(0, 1, 3, 2)
        qm = qf
    else:
        _base._abi_check("osk_attention_fwd_window_anchor_bf16 (fp8)", hd in ((128,) if mode == "qk8" else (72, 128)), vt.dtype == torch.uint8,
                         tuple(vt.shape) == (B, H, _base.vt8_rows(hd), Lp), v_scale is not None and v_scale.numel() == B * H,
                         mode == "pv8" or (k.dtype == torch.uint8 and k_scale is not None and k_scale.numel() == B * H))
        f = vt.view(F8).float()
        assert bool((f[:, :, hd, :Lk] == 1.0).all()) and bool((f[:, :, hd, Lk:] == 0.0).all()), "the validity row is not that of Lk keys"
        vm = f[:, :, :hd, :Lk].permute(0, 1, 3, 2) * v_scale.reshape(B, H, 1, 1)
        if mode == "qk8":
            km = k.view(F8).float()[:, :, :Lk] * k_scale.reshape(B, H, 1, 1)
            amax = qf.abs().amax(-1, keepdim=True)
            s_q = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
            qm = (qf / s_q).clamp(-448.0, 448.0).to(F8).float() * s_q
        else:
            km = k.float().reshape(B, Lk, H, hd).permute(0, 2, 1, 3)
            qm = qf
    if Bq != B:
        idx = torch.arange(Bq) % B
        km, vm = km[idx], vm[idx]
    s_ = (qm @ km.transpose(-1, -2)) * 0.6931471805599453
    if score_bound:
        worst = float(s_.abs().max()) / 0.6931471805599453
        assert worst <= score_bound, f"score bound {score_bound} violated: |score| reaches {worst} (log2 units)"
    s_ = s_.masked_fill(~anchor_mask(Lq, Lk, n_prefix, n_suffix, windows), float("-inf"))
    o = torch.softmax(s_, -1) @ vm
    out.copy_(o.permute(0, 2, 1, 3).reshape(Bq, Lq, D).to(out.dtype))
    if lse is not None:
        lse.copy_(torch.logsumexp(s_, -1))
    return out


def attention_merge_into2(out, lse, o_b, lse_b, o_c, lse_c, H, hd):
    """CPU statement of osk_attention_merge_into2_bf16: f32 weights from the three lse values, f32 sums, one rounding"""
    o, l = merge3_f64(out, lse, o_b, lse_b, o_c, lse_c, H, hd)
    out.copy_(o.to(out.dtype))
    lse.copy_(l.float())
    return out


def merge3_f64(out, lse, o_b, lse_b, o_c, lse_c, H, hd):
    """the three-part merge per element in f64: (out f64 [B, Lq, H*hd], lse f64 [B, H, Lq]); a part at -inf contributes nothing
    (whatever its row holds), all three at -inf: out 0, lse -inf"""
    B, Lq, _ = out.shape
    la, lb, lc = lse.double(), lse_b.double()[:, :, :Lq], lse_c.double()[:, :, :Lq]
    m = torch.maximum(la, torch.maximum(lb, lc))
    ms = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = [torch.exp(x - ms) for x in (la, lb, lc)]                       # exp(-inf) = 0
    tot = e[0] + e[1] + e[2]
    w = [torch.where(tot > 0, x / tot, torch.zeros_like(x)) for x in e]
    parts = [out.double().reshape(B, Lq, H, hd).permute(0, 2, 1, 3), o_b.double()[:, :, :Lq], o_c.double()[:, :, :Lq]]
    acc = sum(torch.where((w_ > 0)[..., None], w_[..., None] * p_, torch.zeros_like(p_)) for w_, p_ in zip(w, parts))
    l = torch.where(tot > 0, ms + torch.log(tot), torch.full_like(tot, float("-inf")))
    return acc.permute(0, 2, 1, 3).reshape(B, Lq, H * hd), l


# ---------------------------------------------------------------------------------------------------------------- the reference
def reference3(q, k, v, H: int, hd: int, n_prefix: int, n_suffix: int, windows: torch.Tensor, kind: str = "bf16"):
    """f64 reference of the anchored entry on prescaled bf16 operands (kind "bf16") or on the e4m3 operands the fp8 kernels multiply
    ("pv8", "qk8"), per query block over exactly that block's stated keys, with the tolerance of the module docstring.  Lq may differ
    from Lk.  Returns dict(out [B, H, Lq, hd], lse [B, H, Lq], tol, lse_tol) in f64."""
    if kind == "bf16":
        qm = R.mfma_q(q, H, hd, 1.0, True, "bf16")
        km, vm = R.mfma_k(k[None], H, hd, "bf16"), R.mfma_v(v[None], H, hd, "bf16")
    else:
        qm, km, vm, _, _ = _F.mfma_operands(q, k, v, H, hd, kind)
    Lq, Lk = q.shape[1], k.shape[1]
    outs = {n_: [] for n_ in ("out", "lse", "tol", "lse_tol")}
    for i, (first, n) in enumerate(windows.tolist()):
        rows = slice(256 * i, min(256 * (i + 1), Lq))
        sets = anchor_key_sets(n_prefix, n_suffix, Lk, first, n)
        keys = torch.cat(sets)
        assert len(keys) == len(set(keys.tolist())), "the three key sets overlap"
        full = R.reference(qm[:, :, rows], km[:, :, keys], vm[:, :, keys], kind)
        parts = [R.reference(qm[:, :, rows], km[:, :, s], vm[:, :, s], kind) for s in sets if len(s)]
        if kind != "bf16":
            assert all(len(s) <= _F.MAX_KEYS for s in sets), "the e4m3 tolerance says nothing beyond 576 keys per launch"
        if len(parts) == 1:
            tol, lse_tol = full["tol"], full["lse_tol"]
        else:
            run = parts[1] if n_prefix else parts[0]                   # launch A's: the only part whose rows are rounded to bf16
            ws = [torch.exp(p["lse"] - full["lse"]) for p in parts]
            assert torch.allclose(sum(w[..., None] * p["out"] for w, p in zip(ws, parts)), full["out"], atol=1e-9)
            wa = torch.exp(run["lse"] - full["lse"])[..., None]
            tol = sum(w[..., None] * p["tol"] for w, p in zip(ws, parts)) + 2.0 ** -9 * wa * run["out"].abs() + 2.0 ** -8 * full["out"].abs()
            lse_tol = sum(w * p["lse_tol"] for w, p in zip(ws, parts)) + (2.0 ** -20 if len(parts) == 3 else 2.0 ** -21) * (1.0 + full["lse"].abs())
        for n_, t in (("out", full["out"]), ("lse", full["lse"]), ("tol", tol), ("lse_tol", lse_tol)):
            outs[n_].append(t)
    return {n_: torch.cat(ts, 2) for n_, ts in outs.items()}
