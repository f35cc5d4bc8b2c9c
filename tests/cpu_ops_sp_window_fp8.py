"""TEST INFRASTRUCTURE ONLY -- tests/cpu_ops_window_anchor.py (and with it the fp8 window entry of tests/cpu_ops_window_fp8.py, the qk8
preparation entries of tests/cpu_ops_sp_qk8.py and the bf16 join of tests/cpu_ops_sp_window.py) plus the CPU statements of
osk_kv_quant_rows_fp8 and osk_kv_join_fp8 (include/osk.h) with the call signatures of open_sora_amd/_C.py: the kernel table of the
host tests of frame-window attention under sequence parallelism in fp8 mode (tests/test_seqpar_window_fp8_host.py).  Every call of
the preparation, join and attention entries is recorded under the calling thread (= the rank of tests/local_transport.py).  As in
tests/cpu_ops.py the e4m3 V^T keeps the natural key order: the order inside a 64-key tile is the kernels' private business.  Never
imported by the product path."""
from __future__ import annotations

import threading

import torch

from tests.cpu_ops_window_anchor import *          # noqa: F401,F403 -- the table is this module's namespace
from tests import cpu_ops as _base
from tests import cpu_ops_sp_qk8 as _Q
from tests import cpu_ops_window_anchor as _A
from tests import cpu_ops_window_fp8 as _F

E4M3 = torch.float8_e4m3fn
U8 = torch.uint8
BF = torch.bfloat16
CALLS: dict = {}      # thread ident -> [(entry name, ...)] in call order
_LOCK = threading.Lock()


def _rec(*desc):
    with _LOCK:
        CALLS.setdefault(threading.get_ident(), []).append(desc)


def kv_quant_rows_fp8(x, scales, out, H, hd):
    """out[b, l, h*hd + d] = e4m3(clamp(x[b, l, h*hd + d] / scales[b, h], +-448)): the arithmetic of k_pack_fp8 / v_transpose_fp8"""
    B, L, D = x.shape
    al = 16 if hd == 128 else 8
    _base._abi_check("osk_kv_quant_rows_fp8", hd in (72, 128), D == H * hd, x.dtype == BF, x.stride(2) == 1, x.stride(0) % 8 == 0,
                     x.stride(1) % 8 == 0, _base._al(x, 16), out.dtype == U8, tuple(out.shape) == (B, L, D), out.stride(2) == 1,
                     out.stride(0) % al == 0, out.stride(1) % al == 0, _base._al(out, al),
                     scales.dtype == torch.float32 and scales.is_contiguous() and scales.numel() == B * H)
    _rec("kv_quant_rows_fp8", B, L, H, hd)
    q = (x.float().reshape(B, L, H, hd) / scales.reshape(B, 1, H, 1)).clamp(-448.0, 448.0).to(E4M3).view(U8)
    out.copy_(q.reshape(B, L, D))
    return out


def kv_join_fp8(k_seg, v_seg, k_out, vt8_out, H, hd, L):
    """key j < L = row j % seg_len of segment j // seg_len.  vt8_out = v_transpose_fp8's layout of those L keys (here: natural key
    order, the 0x38 validity row for keys < L, zeros elsewhere); k_seg uint8 -> k_out = k_pack_fp8's k8 (rows L .. Lp-1 = row L-1);
    k_seg bf16 -> k_out[b, j] = that K row.  The rows of the last segment behind key L - 1 are never read."""
    n_seg, B, seg_len, D = v_seg.shape
    Lp = (L + 63) // 64 * 64
    k8 = k_seg.dtype == U8
    al = 16 if hd == 128 else 8
    _base._abi_check("osk_kv_join_fp8", hd in (72, 128), hd == 128 or not k8, D == H * hd, (n_seg - 1) * seg_len < L <= n_seg * seg_len,
                     v_seg.dtype == U8, v_seg.stride(3) == 1, all(st % al == 0 for st in v_seg.stride()[:3]), _base._al(v_seg, al),
                     tuple(k_seg.shape) == (n_seg, B, seg_len, D), k_seg.stride(3) == 1, k_seg.dtype in (U8, BF),
                     all(st % (16 if k8 else 8) == 0 for st in k_seg.stride()[:3]), _base._al(k_seg, 16), _base._al(k_out, 16),
                     _base._al(vt8_out, 16), vt8_out.dtype == U8, tuple(vt8_out.shape) == (B, H, _base.vt8_rows(hd), Lp), vt8_out.is_contiguous())
    j = torch.arange(L)
    s, r = j // seg_len, j % seg_len
    if k8:
        _base._abi_check("osk_kv_join_fp8 (k8)", k_out.dtype == U8, tuple(k_out.shape) == _Q.k8_shape(B, H, L), k_out.is_contiguous())
        rows = k_seg[s, :, r].reshape(L, B, H, hd).permute(1, 2, 0, 3)              # [B, H, L, 128]
        k_out[:, :, :L] = rows
        k_out[:, :, L:] = rows[:, :, L - 1: L]
    else:
        _base._abi_check("osk_kv_join_fp8 (bf16 K)", k_out.dtype == BF, tuple(k_out.shape) == (B, L, D), k_out.stride(2) == 1,
                         k_out.stride(0) % 8 == 0, k_out.stride(1) % 8 == 0)
        k_out.copy_(k_seg[s, :, r].permute(1, 0, 2))
    _rec("kv_join_fp8", n_seg, seg_len, L, H, "e4m3" if k8 else "bf16")
    vt8_out.zero_()
    vt8_out[:, :, :hd, :L] = v_seg[s, :, r].reshape(L, B, H, hd).permute(1, 2, 3, 0)
    vt8_out[:, :, hd, :L] = 0x38


def kv_scale_fp8(k, v, H, hd, out=None):
    _rec("kv_scale_fp8", k.shape[0], k.shape[1], H)
    return _Q.kv_scale_fp8(k, v, H, hd, out=out)


def v_scale_fp8(v, H, hd):
    _rec("v_scale_fp8", v.shape[0], v.shape[1], H)
    return _base.v_scale_fp8(v, H, hd)


def k_pack_fp8(k, scales, k8, H, hd):
    _rec("k_pack_fp8", k.shape[1], H)
    return _Q.k_pack_fp8(k, scales, k8, H, hd)


def v_transpose_fp8(v, scales, vt8, H, hd):
    _rec("v_transpose_fp8", v.shape[1], H)
    return _base.v_transpose_fp8(v, scales, vt8, H, hd)


def attention_fwd_pv8(q, *a, **kw):
    _rec("attention_fwd_pv8", q.shape[1], kw.get("n_seg", 1), kw.get("seg_len"))
    return _base.attention_fwd_pv8(q, *a, **kw)


def attention_fwd_qk8(q, *a, **kw):
    _rec("attention_fwd_qk8", q.shape[1], kw.get("n_seg", 1), kw.get("seg_len"))
    return _Q.attention_fwd_qk8(q, *a, **kw)


def attention_fwd_ragged(q, *a, **kw):
    _rec("attention_fwd_ragged", q.shape[1], kw.get("n_seg"), kw.get("seg_len"), kw.get("last_seg_len"))
    return _A.attention_fwd_ragged(q, *a, **kw)


def attention_fwd_window_fp8(q, k, k_scale, vt8, v_scale, out, H, hd, scale, *, n_prefix, windows, mode, Lk=None, **kw):
    _rec("attention_fwd_window_fp8", mode, q.shape[1], Lk if mode == "qk8" else k.shape[1], n_prefix, tuple(map(tuple, windows.tolist())),
         None if k_scale is None else k_scale.clone(), v_scale.clone())
    return _F.attention_fwd_window_fp8(q, k, k_scale, vt8, v_scale, out, H, hd, scale, n_prefix=n_prefix, windows=windows, mode=mode, Lk=Lk, **kw)


def attention_fwd_window_anchor(q, k, vt, out, H, hd, scale, *, n_prefix, n_suffix, windows, mode="bf16", Lk=None, **kw):
    _rec("attention_fwd_window_anchor", mode, q.shape[1], Lk if mode == "qk8" else k.shape[1], n_prefix, n_suffix, tuple(map(tuple, windows.tolist())))
    return _A.attention_fwd_window_anchor(q, k, vt, out, H, hd, scale, n_prefix=n_prefix, n_suffix=n_suffix, windows=windows, mode=mode, Lk=Lk, **kw)


# ---------------------------------------------------------------------------------------------------------------- the shared rank cases
RH, RB = 2, 2
R_LT, R_N, R_T = 64, 72, 7                        # 64 text keys + 7 frames x 72 tokens = 568 keys: every key set <= MAX_KEYS for any table
R_L = R_LT + R_N * R_T
_RANK_CASES: dict = {}


def rank_case(kind: str, hd: int, P: int):
    """one rank's quantise -> join -> window path, W = 1: (q, k, v, Lc, [(row0, rows, table, f64 reference over each block's stated
    key set on the e4m3 operands)] per rank), computed once per process and shared by the tests: treat it as read-only"""
    from open_sora_amd.mmdit import attention_window_table

    key = (kind, hd, P)
    if key not in _RANK_CASES:
        q, k, v = _F.operands_fp8(hd, RH, RB, RB, R_L, R_L)
        Lc = -(-R_L // P)
        ranks = []
        for r in range(P):
            row0, rows = r * Lc, min((r + 1) * Lc, R_L) - r * Lc
            t = attention_window_table(R_LT, R_N * R_T, R_N, 1, row0=row0, n_rows=rows)
            ranks.append((row0, rows, t, _F.reference(q[:, row0: row0 + rows].contiguous(), k, v, RH, hd, R_LT, t, kind)))
        _RANK_CASES[key] = (q, k, v, Lc, ranks)
    return _RANK_CASES[key]
