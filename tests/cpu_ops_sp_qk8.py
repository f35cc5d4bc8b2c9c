"""TEST INFRASTRUCTURE ONLY -- the CPU statements of the qk8 entries that tests/cpu_ops.py lacks (osk_kv_scale_fp8, osk_k_pack_fp8,
osk_attention_fwd_qk8_bf16), restating the quantisation rule written in include/osk.h, and an op table that serves them on top of
tests/cpu_ops.py and records, per calling thread (= per rank of tests/local_transport.py), which attention entry ran and with
which scales.  Used by tests/test_seqpar_qk8_host.py and, for the expected bytes, by tests/test_gpu_seqpar_qk8.py."""
from __future__ import annotations

import threading

import torch

from tests import cpu_ops

E4M3 = torch.float8_e4m3fn


def kv_scale_fp8(k, v, H, hd, out=None):
    """osk_kv_scale_fp8: [2, B, H] = (osk_v_scale_fp8 of k, osk_v_scale_fp8 of v)"""
    B = k.shape[0]
    cpu_ops._abi_check("osk_kv_scale_fp8", k.shape == v.shape, hd % 8 == 0, *(t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and
                                                                                t.stride(2) == 1 and cpu_ops._al(t, 16) for t in (k, v)))
    s = torch.stack([cpu_ops.v_scale_fp8(k, H, hd), cpu_ops.v_scale_fp8(v, H, hd)])
    if out is None:
        return s
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (2, B, H)
    return out.copy_(s)


def k8_shape(B, H, L, hd=128):
    assert hd == 128
    return (B, H, (L + 63) // 64 * 64, 128)


def k_pack_fp8(k, scales, k8, H, hd):
    """osk_k_pack_fp8: byte d of row l of head (b, h) = e4m3(clamp(k / scale, +-448)), natural order, rows L .. Lp-1 = row L-1"""
    B, L, _ = k.shape
    cpu_ops._abi_check("osk_k_pack_fp8", hd == 128, k.stride(0) % 8 == 0, k.stride(1) % 8 == 0, cpu_ops._al(k, 16), cpu_ops._al(k8, 16),
                       k8.dtype == torch.uint8 and k8.is_contiguous() and tuple(k8.shape) == k8_shape(B, H, L),
                       scales.dtype == torch.float32 and scales.is_contiguous() and scales.numel() == B * H)
    x = k.float().reshape(B, L, H, hd) / scales.reshape(B, 1, H, 1)
    q = x.clamp(-448.0, 448.0).to(E4M3).view(torch.uint8).permute(0, 2, 1, 3)               # [B, H, L, 128]
    k8[:, :, :L] = q
    k8[:, :, L:] = q[:, :, L - 1: L]
    return k8


def attention_fwd_qk8(q, k8, k_scale, vt8, v_scale, out, H, hd, scale, *, seg_len, lse=None, n_seg=1, k_seg_stride=0, vt_seg_stride=0,
                      q_prescaled=False, kv_batches=0, workspace=None):
    """osk_attention_fwd_qk8_bf16: K from the packed segments times k_scale, Q quantised per (row, head) as the kernel's prologue
    does, then the softmax / P.V statement of osk_attention_fwd_pv8_bf16 on those operands."""
    Bq, Lq, D = q.shape
    B = kv_batches if kv_batches else Bq
    seg_lp = (seg_len + 63) // 64 * 64
    cpu_ops._abi_check("osk_attention_fwd_qk8_bf16", hd == 128, k8.dtype == torch.uint8, tuple(k8.shape) == k8_shape(B, H, seg_len),
                       k_seg_stride % 16 == 0, cpu_ops._al(k8, 16), k_scale.numel() == B * H, v_scale.numel() == B * H,
                       n_seg == 1 or k_seg_stride >= k8.numel())
    K = torch.empty(n_seg, B, seg_len, D)
    for s in range(n_seg):
        seg = torch.as_strided(k8, k8.shape, k8.stride(), k8.storage_offset() + s * k_seg_stride)
        deq = seg.view(E4M3).float()[:, :, :seg_len] * k_scale.reshape(B, H, 1, 1)          # [B, H, seg, 128]
        K[s] = deq.permute(0, 2, 1, 3).reshape(B, seg_len, D)
    qf = q.float().reshape(Bq, Lq, H, hd) * (1.0 if q_prescaled else scale * 1.4426950408889634)
    amax = qf.abs().amax(-1, keepdim=True)
    s_q = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    Q = ((qf / s_q).clamp(-448.0, 448.0).to(E4M3).float() * s_q).reshape(Bq, Lq, D)
    return cpu_ops.attention_fwd_pv8(Q, K[0], vt8, v_scale, out, H, hd, scale, lse=lse, n_seg=n_seg, seg_len=seg_len,
                                     k_seg_stride=K.stride(0), vt_seg_stride=vt_seg_stride, q_prescaled=True, kv_batches=kv_batches)


class Ops:
    """tests/cpu_ops.py plus the entries above; every attention call is recorded under the calling thread"""

    def __init__(self):
        self._lock = threading.Lock()
        self.qk8_calls: dict = {}     # thread ident -> [(k_scale, v_scale) clones, one per call]
        self.pv8_calls: dict = {}     # thread ident -> number of calls

    def __getattr__(self, name):
        return getattr(cpu_ops, name)

    kv_scale_fp8 = staticmethod(kv_scale_fp8)
    k8_shape = staticmethod(k8_shape)
    k_pack_fp8 = staticmethod(k_pack_fp8)

    def attention_fwd_qk8(self, q, k8, k_scale, vt8, v_scale, out, H, hd, scale, **kw):
        with self._lock:
            self.qk8_calls.setdefault(threading.get_ident(), []).append((k_scale.clone(), v_scale.clone()))
        return attention_fwd_qk8(q, k8, k_scale, vt8, v_scale, out, H, hd, scale, **kw)

    def attention_fwd_pv8(self, *a, **kw):
        with self._lock:
            t = threading.get_ident()
            self.pv8_calls[t] = self.pv8_calls.get(t, 0) + 1
        return cpu_ops.attention_fwd_pv8(*a, **kw)
