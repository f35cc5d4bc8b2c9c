"""TEST INFRASTRUCTURE ONLY -- tests/cpu_ops_step_cache.py plus the CPU statement of osk_step_sums_combine_f32 (include/osk.h), with
the call signature of open_sora_amd/_C.py, and its plain f64 reference: the kernel table of the step cache under sequence
parallelism.  The ranks of the host tests run as threads (tests/local_transport.py), so the calls are recorded per thread.  Never
imported by the product path."""
from __future__ import annotations

import threading

import torch

from tests.cpu_ops_step_cache import *          # noqa: F401,F403 -- the table is this module's namespace
from tests import cpu_ops as _base
from tests.cpu_ops_ragged import attention_fwd_ragged, attention_ragged_workspace    # noqa: F401 -- a ragged split's attention entry
from tests.cpu_ops_sp_chunked import attention_merge                                  # noqa: F401 -- kv_chunks > 1: the merge of the slices

SP_CALLS: dict = {}     # thread ident -> [(entry, P)] of that rank's step_sums_combine calls


def step_sums_combine(pairs, sums):
    """sums[j] = ((pairs[0][j] + pairs[1][j]) + ...) + pairs[P-1][j]: f32 adds one after the other, in row order"""
    lo, hi = pairs.data_ptr(), pairs.data_ptr() + 4 * pairs.numel()
    _base._abi_check("osk_step_sums_combine_f32", pairs.dtype == torch.float32 and pairs.ndim == 2 and pairs.shape[0] >= 1,
                     pairs.shape[1] == 2 and pairs.is_contiguous(), sums.dtype == torch.float32 and sums.numel() == 2 and sums.is_contiguous(),
                     _base._al(pairs, 4) and _base._al(sums, 4), not (sums.data_ptr() < hi and lo < sums.data_ptr() + 8))
    SP_CALLS.setdefault(threading.get_ident(), []).append(("step_sums_combine", pairs.shape[0]))
    acc = pairs[0].clone()
    for r in range(1, pairs.shape[0]):
        acc = acc + pairs[r]                    # an f32 tensor add: one rounding per element, no reassociation
    sums.copy_(acc)
    return sums


def step_sums_combine_f64(pairs: torch.Tensor) -> tuple[float, float]:
    """the two column sums of f32 [P, 2] in f64"""
    s = pairs.to(torch.float64).sum(0)
    return float(s[0]), float(s[1])
