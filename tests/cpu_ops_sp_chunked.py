"""TEST INFRASTRUCTURE ONLY -- the CPU statement of osk_attention_merge_bf16 (include/osk.h), which tests/cpu_ops.py lacks, an f64
statement of the same merge (the reference of tests/test_gpu_attention_merge.py), and an op table that serves the CPU statement
on top of tests/cpu_ops.py and records, per calling thread (= per rank of tests/local_transport.py), the sequence of op calls.
Used by tests/test_seqpar_chunked_host.py and the GPU tests of the chunked gather."""
from __future__ import annotations

import threading

import torch

from tests import cpu_ops


def attention_merge(parts, lse, out, H, hd, lse_out=None):
    """osk_attention_merge_bf16: f32 weights and sums, ONE rounding to bf16; a part with lse = -inf weighs 0, all of them: zeros"""
    S, B, L, D = parts.shape
    cpu_ops._abi_check("osk_attention_merge_bf16", 1 <= S <= 8, hd % 8 == 0, D == H * hd, parts.stride(3) == 1, out.stride(2) == 1,
                       all(st % 8 == 0 for st in parts.stride()[:3]), all(st % 8 == 0 for st in out.stride()[:2]),
                       cpu_ops._al(parts, 16), cpu_ops._al(out, 16), tuple(lse.shape) == (S, B, H, L), lse.is_contiguous(),
                       lse.dtype == torch.float32, tuple(out.shape) == (B, L, D),
                       lse_out is None or (lse_out.is_contiguous() and tuple(lse_out.shape) == (B, H, L)))
    m = lse.amax(0)                                                             # [B, H, L]
    w = torch.where(torch.isinf(lse) & (lse < 0), torch.zeros_like(lse), (lse - m).exp())
    tot = w.sum(0)
    wn = torch.where(tot > 0, w / tot, torch.zeros_like(w))                     # [S, B, H, L]
    p = parts.float().reshape(S, B, L, H, hd)
    o = (wn.permute(0, 1, 3, 2).unsqueeze(-1) * p).sum(0).reshape(B, L, D)
    out.copy_(o.to(out.dtype))
    if lse_out is not None:
        lse_out.copy_(torch.where(tot > 0, m + tot.log(), torch.full_like(m, float("-inf"))))
    return out


def attention_merge_f64(parts, lse):
    """the merge in f64 on the SAME bf16 partials and f32 lse values: (exact [B, L, D], lse_out [B, H, L],
    sum_s wbar_s |part_s| [B, L, D] -- the magnitude the f32 accumulation error of the kernel scales with)"""
    S, B, L, D = parts.shape
    H = lse.shape[2]
    l64 = lse.double()
    m = l64.amax(0)
    w = torch.where(torch.isinf(l64) & (l64 < 0), torch.zeros_like(l64), (l64 - m).exp())
    tot = w.sum(0)
    wn = torch.where(tot > 0, w / tot, torch.zeros_like(w)).permute(0, 1, 3, 2).unsqueeze(-1)    # [S, B, L, H, 1]
    p = parts.double().reshape(S, B, L, H, D // H)
    exact = (wn * p).sum(0).reshape(B, L, D)
    mag = (wn * p.abs()).sum(0).reshape(B, L, D)
    lse_out = torch.where(tot > 0, m + tot.log(), torch.full_like(m, float("-inf")))
    return exact, lse_out, mag


class Ops:
    """tests/cpu_ops.py plus attention_merge; every call of an op that the sequence-parallel exchange issues is recorded under the
    calling thread as (name, shapes of the positional tensors, keyword scalars that shape the launch, shapes of the keyword tensors)"""

    RECORDED = ("copy_rows", "v_transpose", "attention_fwd", "attention_merge", "attention_fwd_pv8", "v_transpose_fp8", "v_scale_fp8")

    def __init__(self):
        self._lock = threading.Lock()
        self.calls: dict = {}         # thread ident -> [(name, ...)]

    def _rec(self, name, a, kw):
        desc = (name, tuple(tuple(x.shape) for x in a if isinstance(x, torch.Tensor)),
                tuple(sorted((k, v) for k, v in kw.items() if isinstance(v, (int, float, bool)))),
                tuple(sorted((k, tuple(v.shape)) for k, v in kw.items() if isinstance(v, torch.Tensor) and k != "workspace")))
        with self._lock:
            self.calls.setdefault(threading.get_ident(), []).append(desc)

    def __getattr__(self, name):
        fn = attention_merge if name == "attention_merge" else getattr(cpu_ops, name)
        if name not in self.RECORDED:
            return fn

        def recorded(*a, **kw):
            self._rec(name, a, kw)
            return fn(*a, **kw)

        return recorded
