"""TEST INFRASTRUCTURE ONLY -- tests/cpu_ops_step_cache_sp.py plus the CPU statement of osk_attn_cache_copy_bf16 (include/osk.h), with
the call signature of open_sora_amd/_C.py: the kernel table of the sampler's attention broadcast, sharded or not.  Also a tracing
wrapper around a kernel table that records every call as (entry, shapes of its tensor arguments).  The ranks of the sharded host
tests run as threads (tests/local_transport.py), so calls are recorded per thread.  Never imported by the product path."""
from __future__ import annotations

import threading

import torch

from tests.cpu_ops_step_cache_sp import *          # noqa: F401,F403 -- the table is this module's namespace
from tests import cpu_ops as _base

BF = torch.bfloat16
AB_CALLS: dict = {}     # thread ident -> [("store" | "load", batch items, rows of the map or None)]


def _view_ok(t) -> bool:
    return (t.dtype == BF and t.ndim == 3 and t.numel() > 0 and t.shape[2] % 8 == 0 and t.stride(2) == 1 and t.stride(0) % 8 == 0
            and t.stride(1) % 8 == 0 and _base._al(t, 16))


def attn_cache_copy(src, dst, row_map, to_cache):
    """store: dst[row_map[b]] = src[b]; load: dst[b] = src[row_map[b]]; row_map None = the identity.  A map entry outside the slot
    skips the batch item, as the kernel does."""
    step, slot = (src, dst) if to_cache else (dst, src)
    B = step.shape[0]
    _base._abi_check("osk_attn_cache_copy_bf16", _view_ok(src), _view_ok(dst), slot.shape[1:] == step.shape[1:],
                     row_map is not None or B <= slot.shape[0],
                     row_map is None or (row_map.dtype == torch.int32 and row_map.ndim == 1 and row_map.numel() == B),
                     all(t.shape[0] == 1 or t.stride(0) >= t.shape[1] * t.stride(1) for t in (src, dst)))
    rows = list(range(B)) if row_map is None else [int(r) for r in row_map.tolist()]
    AB_CALLS.setdefault(threading.get_ident(), []).append(("store" if to_cache else "load", B, None if row_map is None else tuple(rows)))
    for b, r in enumerate(rows):
        if 0 <= r < slot.shape[0]:
            if to_cache:
                dst[r].copy_(src[b])
            else:
                dst[b].copy_(src[r])
    return dst


# ----------------------------------------------------------------------------- a tracing wrapper around a kernel table
def _shapes(v):
    if torch.is_tensor(v):
        return tuple(v.shape)
    if isinstance(v, dict):
        return tuple(sorted((k, _shapes(x)) for k, x in v.items() if torch.is_tensor(x)))
    if isinstance(v, (list, tuple)):
        s = tuple(_shapes(x) for x in v)
        return tuple(x for x in s if x is not None) or None
    return None


class Traced:
    """a kernel table that forwards to `table` and appends (entry, shapes of the tensor arguments -- positional, then keyword by name;
    the operand dicts of gemm_pair / gemm_group by key) to `log` for every call of a function of the table; classes (GemvTasks) and
    constants pass through.  Query-only entries in `quiet` are not recorded."""

    quiet = ("copy_rows_ok", "gemm_fp8_supported", "attention_workspace", "vt8_rows", "k8_shape", "step_delta_workspace_bytes")

    def __init__(self, table, log: list):
        self._table, self._log = table, log

    def __getattr__(self, name):
        v = getattr(self._table, name)             # AttributeError for a missing entry: hasattr() answers as the table does
        if not callable(v) or isinstance(v, type) or name in self.quiet or name.startswith("_"):
            return v

        def traced(*a, **k):
            shapes = tuple(s for s in (_shapes(x) for x in a) if s is not None)
            shapes += tuple((key, _shapes(x)) for key, x in sorted(k.items()) if _shapes(x) is not None)
            self._log.append((name, shapes))
            return v(*a, **k)

        return traced
