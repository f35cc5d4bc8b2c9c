"""TEST INFRASTRUCTURE ONLY -- tests/cpu_ops_window.py plus the CPU statement of osk_kv_join_bf16 (include/osk.h) with the call signature
of open_sora_amd/_C.py: the kernel table of the host tests of frame-window attention under sequence parallelism
(tests/test_seqpar_window_host.py).  Every kv_join and attention_fwd_window call is recorded under the calling thread (= the rank of
tests/local_transport.py).  Never imported by the product path."""
from __future__ import annotations

import threading

import torch

from tests.cpu_ops_window import *          # noqa: F401,F403 -- the table is this module's namespace
from tests import cpu_ops as _base
from tests import cpu_ops_window as _W
from tests.cpu_ops_ragged import attention_fwd_ragged, attention_ragged_workspace    # noqa: F401 -- a ragged split with the window off

CALLS: dict = {}      # thread ident -> [("kv_join", n_seg, seg_len, L, H) | ("attention_fwd_window", Lq, Lk, n_prefix, score_bound, table rows)]
_LOCK = threading.Lock()


def _rec(*desc):
    with _LOCK:
        CALLS.setdefault(threading.get_ident(), []).append(desc)


def kv_join(k_seg, v_seg, k_out, vt_out, H, hd, L):
    """key j < L = row j % seg_len of segment j // seg_len; k_out[b, j] = that K row, vt_out[b, h, d, p] = V of key(p) (the position
    -> key map of osk_v_transpose_bf16 inside every 64-key tile) or zero where key(p) >= L.  The rows of the last segment behind
    key L - 1 are never read."""
    n_seg, B, seg_len, D = k_seg.shape
    Lp = (L + 63) // 64 * 64
    _base._abi_check("osk_kv_join_bf16", hd in (64, 72, 128), D == H * hd, (n_seg - 1) * seg_len < L <= n_seg * seg_len,
                     v_seg.shape == k_seg.shape, v_seg.stride() == k_seg.stride(), k_seg.stride(3) == 1, k_out.stride(2) == 1,
                     all(st % 8 == 0 for st in k_seg.stride()[:3]), all(st % 8 == 0 for st in k_out.stride()[:2]),
                     _base._al(k_seg, 16), _base._al(v_seg, 16), _base._al(k_out, 16), _base._al(vt_out, 16),
                     tuple(k_out.shape) == (B, L, D), tuple(vt_out.shape) == (B, H, hd, Lp), vt_out.is_contiguous())
    _rec("kv_join", n_seg, seg_len, L, H)
    j = torch.arange(L)
    s, r = j // seg_len, j % seg_len
    k_out.copy_(k_seg[s, :, r].permute(1, 0, 2))                                   # [L, B, D] -> [B, L, D]
    key = _base.pos2key(hd, Lp)                                                    # key stored at position p
    valid = key < L
    kc = key.clamp(max=L - 1)
    vp = v_seg[kc // seg_len, :, kc % seg_len]                                     # [Lp, B, D]
    vp = torch.where(valid[:, None, None], vp, torch.zeros_like(vp))
    vt_out.copy_(vp.reshape(Lp, B, H, hd).permute(1, 2, 3, 0))


def attention_fwd_window(q, k, vt, out, H, hd, scale, *, n_prefix, windows, **kw):
    _rec("attention_fwd_window", q.shape[1], k.shape[1], n_prefix, float(kw.get("score_bound", 0.0)), tuple(map(tuple, windows.tolist())))
    return _W.attention_fwd_window(q, k, vt, out, H, hd, scale, n_prefix=n_prefix, windows=windows, **kw)
