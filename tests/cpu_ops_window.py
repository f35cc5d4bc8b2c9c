"""TEST INFRASTRUCTURE ONLY -- tests/cpu_ops.py plus the CPU statement of the frame-window attention entry (include/osk.h,
osk_attention_fwd_window_bf16) with the call signatures of open_sora_amd/_C.py: a kernel table for mmdit.set_ops_for_testing().
Beside it, what the tests of that entry share: operands, the f64 reference over exactly each query block's key set with the derived
tolerance, and a torch emulation of the two launches and the merge.  Never imported by the product path.

Tolerance (derived, not fitted).  n_prefix == 0: launch A alone, the tolerance of tests/cpu_ops_attn_f64.reference on the block's keys.
n_prefix > 0: out = w_A O_A + w_B O_B with the f64 merge weights w_A + w_B = 1, O_A the window-only and O_B the prefix-only output:
    tol = w_A tol_A + w_B tol_B + 2^-9 w_A |O_A| + 2^-8 |ref|
the two launches' own tolerances, launch A's bf16 rounding of its finished rows, and the final rounding.  The merged LSE is
log(e^lse_A + e^lse_B): d lse = w_A d lse_A + w_B d lse_B, plus 2^-21 (1 + |lse|) for the f32 exp / log / sum of the merge kernel."""
from __future__ import annotations

import math

import torch

from tests.cpu_ops import *          # noqa: F401,F403 -- the table is this module's namespace
from tests import cpu_ops as _base
from tests import cpu_ops_attn_f64 as R
from tests.cpu_ops_cfg_prune import cfg_euler_nb    # noqa: F401 -- the sampler's pruned loop (cpu_ops lacks it)

BF = torch.bfloat16
WINDOW_CALLS = []     # (n_prefix, score_bound, table as a tuple of rows) of every call: the tests read which path a forward took


def attention_window_workspace_bytes(B, H, Lq, hd):
    return 16


def attention_window_workspace(B, H, Lq, hd, device):
    return torch.empty(16, dtype=torch.uint8, device=device)


def block_keys(n_prefix: int, Lk: int, first: int, n: int) -> torch.Tensor:
    """key indices a query block with table row (first, n) sees: the prefix and body tiles [first, first + n), cut at Lk"""
    a, b = n_prefix + 64 * first, min(n_prefix + 64 * (first + n), Lk)
    return torch.cat([torch.arange(n_prefix), torch.arange(a, b)])


def window_mask(Lq: int, Lk: int, n_prefix: int, windows: torch.Tensor) -> torch.Tensor:
    """bool [Lq, Lk]: the block-granular mask the entry states"""
    m = torch.zeros(Lq, Lk, dtype=torch.bool)
    for i, (first, n) in enumerate(windows.tolist()):
        m[256 * i: 256 * (i + 1), block_keys(n_prefix, Lk, first, n)] = True
    return m


def attention_fwd_window(q, k, vt, out, H, hd, scale, *, n_prefix, windows, lse=None, q_prescaled=False, kv_batches=0,
                         score_bound=0.0, workspace=None):
    """dense f32 scores with the block-granular mask, one softmax, one rounding"""
    Bq, Lq, D = q.shape
    Lk = k.shape[1]
    B = kv_batches if kv_batches else Bq
    nqb, tiles = (Lq + 255) // 256, (Lk - n_prefix + 63) // 64
    _base._abi_check("osk_attention_fwd_window_bf16", q.stride(0) % 8 == 0, q.stride(1) % 8 == 0, k.stride(0) % 8 == 0, k.stride(1) % 8 == 0,
                     _base._al(q, 16), _base._al(k, 16), _base._al(vt, 16), 0 <= kv_batches <= Bq, n_prefix % 64 == 0, 0 <= n_prefix < Lk,
                     tuple(windows.shape) == (nqb, 2), windows.dtype == torch.int32, score_bound >= 0,
                     n_prefix == 0 or (workspace is not None and out.stride(0) % 8 == 0 and out.stride(1) % 8 == 0 and _base._al(out, 16)))
    if bool((windows[:, 0] < 0).any()) or bool((windows[:, 1] < 1).any()) or bool((windows[:, 0] + windows[:, 1] > tiles).any()):
        raise ValueError("windows: a range outside the body's tiles")
    WINDOW_CALLS.append((n_prefix, float(score_bound), tuple(map(tuple, windows.tolist()))))
    Lp = (Lk + 63) // 64 * 64
    key2pos = torch.empty(Lp, dtype=torch.long)
    key2pos[_base.pos2key(hd, Lp)] = torch.arange(Lp)
    K = k.float().reshape(B, Lk, H, hd).permute(0, 2, 1, 3)
    V = vt.float().reshape(B, H, hd, Lp)[..., key2pos][..., :Lk].permute(0, 1, 3, 2)
    Q = q.float().reshape(Bq, Lq, H, hd).permute(0, 2, 1, 3)
    if Bq != B:
        idx = torch.arange(Bq) % B
        K, V = K[idx], V[idx]
    s_ = (Q @ K.transpose(-1, -2)) * (0.6931471805599453 if q_prescaled else scale)
    if score_bound:
        worst = float(s_.abs().max()) / 0.6931471805599453
        assert worst <= score_bound, f"score bound {score_bound} violated: |score| reaches {worst} (log2 units)"
    s_ = s_.masked_fill(~window_mask(Lq, Lk, n_prefix, windows), float("-inf"))
    o = torch.softmax(s_, -1) @ V
    out.copy_(o.permute(0, 2, 1, 3).reshape(Bq, Lq, D).to(out.dtype))
    if lse is not None:
        lse.copy_(torch.logsumexp(s_, -1))
    return out


# ---------------------------------------------------------------------------------------------------------------- test operands
def operands(hd: int, H: int, B: int, Bkv: int, L: int, seed: int = 0, bound: float = 48.0):
    """q (prescaled, log2 units), k, v bf16 [B | Bkv, L, H*hd] for Lq = Lk = L, and a score bound that holds: scores with a
    standard deviation of several log2 units -- a row's mass sits on a few keys, so a window that moves by a tile moves the
    output -- under max |q| max |k| * 1.01 <= `bound` (the FAST body's limit is 56)."""
    g = torch.Generator().manual_seed(1000 * hd + 10 * L + Bkv + seed)
    k = torch.randn(Bkv, L, H * hd, generator=g).to(BF)
    v = torch.randn(Bkv, L, H * hd, generator=g).to(BF)
    q = torch.randn(B, L, H * hd, generator=g)
    kn = k.float().reshape(Bkv, L, H, hd).norm(dim=-1).max()
    qn = q.reshape(B, L, H, hd).norm(dim=-1).max()
    q = (q * (bound / 1.02 / float(qn * kn))).to(BF)
    qn = q.float().reshape(B, L, H, hd).norm(dim=-1).max()
    sb = float(qn * kn) * 1.01
    assert sb <= bound, sb
    return q, k, v, sb


def reference(q, k, v, H: int, hd: int, n_prefix: int, windows: torch.Tensor):
    """f64 reference of the entry on prescaled bf16 operands, per query block over exactly that block's keys, with the tolerance of
    the module docstring.  Returns dict(out [B, H, Lq, hd], lse [B, H, Lq], tol, lse_tol) in f64."""
    qm = R.mfma_q(q, H, hd, 1.0, True, "bf16")
    km, vm = R.mfma_k(k[None], H, hd, "bf16"), R.mfma_v(v[None], H, hd, "bf16")
    Lq, Lk = q.shape[1], k.shape[1]
    outs = {n_: [] for n_ in ("out", "lse", "tol", "lse_tol")}
    for i, (first, n) in enumerate(windows.tolist()):
        rows = slice(256 * i, min(256 * (i + 1), Lq))
        keys = block_keys(n_prefix, Lk, first, n)
        full = R.reference(qm[:, :, rows], km[:, :, keys], vm[:, :, keys], "bf16")
        if n_prefix == 0:
            tol, lse_tol = full["tol"], full["lse_tol"]
        else:
            a = R.reference(qm[:, :, rows], km[:, :, keys[n_prefix:]], vm[:, :, keys[n_prefix:]], "bf16")
            b = R.reference(qm[:, :, rows], km[:, :, :n_prefix], vm[:, :, :n_prefix], "bf16")
            wa, wb = torch.exp(a["lse"] - full["lse"])[..., None], torch.exp(b["lse"] - full["lse"])[..., None]
            assert torch.allclose(wa * a["out"] + wb * b["out"], full["out"], atol=1e-9)
            tol = wa * a["tol"] + wb * b["tol"] + 2.0 ** -9 * wa * a["out"].abs() + 2.0 ** -8 * full["out"].abs()
            lse_tol = wa[..., 0] * a["lse_tol"] + wb[..., 0] * b["lse_tol"] + 2.0 ** -21 * (1.0 + full["lse"].abs())
        for n_, t in (("out", full["out"]), ("lse", full["lse"]), ("tol", tol), ("lse_tol", lse_tol)):
            outs[n_].append(t)
    return {n_: torch.cat(ts, 2) for n_, ts in outs.items()}


def emulate(q, k, v, H: int, hd: int, n_prefix: int, windows: torch.Tensor, m_mode, drop_prefix: bool = False):
    """the entry as the kernels compute it (tests/cpu_ops_attn_f64.emulate per launch): launch A over the block's window into bf16
    rows and an f32 lse, launch B over the prefix into an f32 partial, the merge in f32 with one rounding.  drop_prefix: the merge
    never happens (a mutant).  Returns (out f32 [B, H, Lq, hd] holding bf16 values, lse f32 [B, H, Lq])."""
    qm = R.mfma_q(q, H, hd, 1.0, True, "bf16")
    km, vm = R.mfma_k(k[None], H, hd, "bf16"), R.mfma_v(v[None], H, hd, "bf16")
    Lq, Lk = q.shape[1], k.shape[1]
    outs, lses = [], []
    for i, (first, n) in enumerate(windows.tolist()):
        rows = slice(256 * i, min(256 * (i + 1), Lq))
        keys = block_keys(n_prefix, Lk, first, n)[n_prefix:]
        oa, la = R.emulate(qm[:, :, rows], km[:, :, keys], vm[:, :, keys], "bf16", m_mode)
        if n_prefix and not drop_prefix:
            # the partial of launch B: two equal parts of which the "merge" sums one = the normalised f32 partial, before any rounding
            idx = torch.arange(q.shape[0]) % km.shape[0]
            s = qm[:, :, rows].float() @ km.float()[idx][:, :, :n_prefix].transpose(-1, -2)
            m = s.amax(-1, keepdim=True) if isinstance(m_mode, str) else torch.full_like(s[..., :1], float(m_mode))
            p = torch.exp2(s - m).to(BF).float()
            den = p.sum(-1, keepdim=True)
            ob, lb = (p @ vm.float()[idx][:, :, :n_prefix]) / den, ((m + torch.log2(den)) * R.LN2).squeeze(-1)
            mm = torch.maximum(la, lb)
            ea, eb = torch.exp(la - mm), torch.exp(lb - mm)
            tot = ea + eb
            oa = ((ea / tot)[..., None] * oa + (eb / tot)[..., None] * ob).to(BF).float()
            la = mm + torch.log(tot)
        outs.append(oa)
        lses.append(la)
    return torch.cat(outs, 2), torch.cat(lses, 2)


def hand_table(Lq: int, body: int) -> torch.Tensor:
    """a table with a 1-tile range, a 2-tile range, a range that ends in the body's last (possibly ragged) tile, one that ends
    before it and, where a fifth block exists, the last tile alone"""
    tiles = (body + 63) // 64
    rows = [(3, 1), (5, 2), (tiles - 3, 3), (2, tiles - 3), (tiles - 1, 1)]
    return torch.tensor(rows[: (Lq + 255) // 256], dtype=torch.int32)


assert math.isclose(R.LN2, math.log(2.0))
