"""ctypes binding of libosk_hip.so (include/osk.h).  No torch types cross the boundary: tensors are
unwrapped to (data_ptr, strides) here; the stream is torch's current HIP stream.

There is NO fallback: if the library is missing or an entry point is absent the import fails loudly,
and a non-zero status from a kernel launch raises RuntimeError (binding layer translates C status ->
Python exception, SURVEY.md §8(b) "Error conventions").
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from .build import LIB_PATH

_i64, _i32, _f32, _f64, _vp = C.c_int64, C.c_int32, C.c_float, C.c_double, C.c_void_p

# symbol -> argtypes, exactly the declarations of include/osk.h
SIGNATURES = {
    "osk_abi_version": [],
    "osk_arch": [],
    "osk_gemm_geglu_bf16": [_vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _i64, _vp],
    "osk_attention_short_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32,
                                 _f32, _vp],
    "osk_attention_relbias_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i32, _i32, _i32, _i32,
                                   _f32, _vp],
    "osk_attention_kernel_name": [_i32, _i32],
    "osk_attention_body_name": [_i32, _i32, _i32, _f32],
    "osk_ln_modulate_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _vp],
    "osk_gemm_bf16": [_vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _i64,
                      _i32, _i32, _i32, _i32, _i32, _vp],
    "osk_gemm_bf16_pair": [_vp, _vp, _i32, _i32, _i32, _vp],     # two OskGemmOperands structs by pointer
    "osk_gemm_group_bf16": [_vp, _i32, _i32, _vp],              # OskGemmTask array by pointer
    "osk_gemm_tile_choice": [_i32, _i32, _i32],
    "osk_gemm_tile_choice_strided": [_i32, _i32, _i32, _i64, _i64, _i32, _i64],
    "osk_gemm_tile_override": [_i32],
    "osk_ln_modulate_fp8": [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _vp],
    "osk_quantize_rows_fp8": [_vp, _i64, _i64, _i32, _vp, _vp, _i32, _i32, _vp],
    "osk_gemm_fp8": [_vp, _i64, _i64, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _i64,
                     _i32, _i32, _i32, _i32, _i32, _vp],
    "osk_gemv_tasks_bf16": [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _i32, _i32, _vp],
    "osk_timestep_embedding": [_vp, _i32, _i32, _f32, _f32, _vp, _vp],
    "osk_rope_table": [_vp, _i64, _i32, C.POINTER(_i32), _f64, _i32, _vp, _vp, _vp],
    "osk_qknorm_rope_bf16": [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i64,
                             _i32, _i32, _i32, _i32, _i32, _f32, _f32, _vp],
    "osk_v_transpose_bf16": [_vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _vp],
    "osk_kv_join_bf16": [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    "osk_kv_quant_rows_fp8": [_vp, _i64, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp],
    "osk_kv_join_fp8": [_vp, _i64, _i64, _i64, _i32, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    "osk_attention_fwd_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _vp,
                               _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _i32, _vp],
    "osk_attention_fwd_ws_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _vp,
                                  _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _i32, _vp, _i64, _vp],
    "osk_attention_fwd_bounded_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _vp,
                                       _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _i32, _f32, _vp, _i64, _vp],
    "osk_attention_fwd_auto_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _vp,
                                    _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _i32, _vp, _vp, _vp, _i64, _vp],
    "osk_attention_merge_bf16": [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    "osk_attention_ragged_workspace_bytes": [_i32, _i32, _i32, _i32],
    "osk_attention_fwd_ragged_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i64, _vp,
                                      _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _i32, _f32, _i32, _vp, _i64, _vp],
    "osk_attention_merge_into_bf16": [_vp, _i64, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "osk_attention_window_workspace_bytes": [_i32, _i32, _i32, _i32],
    "osk_attention_fwd_window_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _i32,
                                      _f32, _i32, _i32, _f32, _vp, _i32, _vp, _i64, _vp],
    "osk_attention_fwd_window_fp8_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32,
                                          _i32, _i32, _f32, _i32, _i32, _i32, _vp, _i32, _vp, _i64, _vp],
    "osk_attention_merge_into2_bf16": [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "osk_attention_window_anchor_workspace_bytes": [_i32, _i32, _i32, _i32],
    "osk_attention_fwd_window_anchor_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32,
                                             _i32, _i32, _i32, _f32, _i32, _i32, _f32, _i32, _vp, _i32, _vp, _i64, _vp],
    "osk_rownorm2_max_bf16": [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _i32, _vp],
    "osk_attention_workspace_bytes": [],
    "osk_v_scale_fp8": [_vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _vp],
    "osk_kv_scale_fp8": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _vp],
    "osk_v_transpose_fp8": [_vp, _i64, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "osk_attention_fwd_pv8_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _vp,
                                   _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _i32, _vp, _i64, _vp],
    "osk_k_pack_fp8": [_vp, _i64, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "osk_attention_fwd_qk8_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i64, _vp,
                                   _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _i32, _vp, _i64, _vp],
    "osk_attention_tail_split_factor": [_i32, _i32, _i32, _i32, _i32, _i32, _i64],
    "osk_attention_launch_shape": [_i32, _i32, _i32, _i32, _i32, _i32, _f32, _i64, C.POINTER(_i32)],
    "osk_attention_rows_override": [_i32],
    "osk_cfg_euler_bf16": [_vp, _i64, _vp, _vp, _f32, _f32, _vp, _f32, _vp],
    "osk_cfg_euler_nb_bf16": [_vp, _i32, _i64, _vp, _vp, _f32, _f32, _vp, _f32, _vp],
    "osk_copy_rows_bf16": [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _vp],
    "osk_step_delta_workspace_bytes": [_i32, _i32, _i32],
    "osk_step_delta_bf16": [_vp, _i64, _i64, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _vp],
    "osk_step_sums_combine_f32": [_vp, _i32, _vp, _vp],
    "osk_residual_sub_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _vp],
    "osk_residual_add_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _vp],
    "osk_attn_cache_copy_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    "osk_causal_conv3d_ndhwc_bf16": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32,
                                     _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp],
    "osk_causal_conv3d_gn_ndhwc_bf16": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32,
                                        _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp],
    "osk_causal_conv3d_kernel_class": [_i32, _i32, _i32, _i32, _i32, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                       _i32, _i32, _i32, _i32, _i32],
    "osk_causal_conv3d_gnin_ndhwc_bf16": [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _i32, _i32, _i32, _i32,
                                          _i32, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp],
    "osk_conv2d_nhwc_bf16": [_vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32,
                             _vp, _i32, _vp],
    "osk_groupnorm_table_f32": [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _f32, _vp],
    "osk_groupnorm_stats_ndhwc_bf16": [_vp, _i32, _i64, _i32, _i32, _vp, _vp],
    "osk_groupnorm_apply_ndhwc_bf16": [_vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _f32, _i32, _vp],
    "osk_masked_softmax_f32_bf16": [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _f32, _vp],
    "osk_blend_bf16": [_vp, _vp, _i64, _i32, _i32, _i32, _i64, _vp],
    "osk_attention_hd512_fwd_ws_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _i32, _i32,
                                        _i32, _f32, _vp, _i64, _vp],
    "osk_attention_hd512_workspace_bytes": [_i32, _i32],
    "osk_attention_hd512_fwd_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _i32, _i32,
                                     _i32, _f32, _vp],
    "osk_conv3d_zp_ndhwc_bf16": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp],
    "osk_conv3d_zp_strided_ndhwc_bf16": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    "osk_dup_shuffle_ndhwc_bf16": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _vp],
    "osk_unshuffle_avg_ndhwc_bf16": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _vp],
    "osk_dwconv3d_ndhwc_bf16": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp],
    "osk_gconv32_bf16": [_vp, _i64, _i32, _vp, _vp, _vp],
    "osk_relu_linear_attn_bf16": [_vp, _i32, _i32, _i32, _vp, _i64, _vp, _i64, _i32, _f32, _vp],
    "osk_rmsnorm_affine_bf16": [_vp, _i64, _i32, _vp, _vp, _f32, _vp, _i32, _vp, _vp],
    "osk_layernorm_affine_bf16": [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _f32, _vp],
    "osk_attention_causal_bf16": [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _f32, _vp],
    "osk_gemm_quickgelu_bf16": [_vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp],
    "osk_lora_merge_bf16": [_vp, _i64, _vp, _i64, _i32, _i32, _vp, _i32, _vp],     # OskLoraAdapter array (host) by pointer
}


def _load() -> C.CDLL:
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m open_sora_amd.build` (hipcc, gfx950). "
            "open_sora_amd has no CPU or eager fallback."
        )
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.argtypes = argtypes
        fn.restype = (C.c_char_p if name in ("osk_arch", "osk_attention_kernel_name", "osk_attention_body_name") else
                      _i64 if name in ("osk_attention_workspace_bytes", "osk_attention_hd512_workspace_bytes",
                                       "osk_attention_ragged_workspace_bytes", "osk_attention_window_workspace_bytes",
                                       "osk_attention_window_anchor_workspace_bytes",
                                       "osk_step_delta_workspace_bytes") else _i32)
    if lib.osk_abi_version() != 2:
        raise ImportError("libosk_hip.so ABI version mismatch")
    return lib


class _TracingLib:
    """OSK_TRACE=1: every C-ABI call is recorded in TRACE_LOG as (entry point, arguments) before it is forwarded.  A pointer is
    replaced by 'p<k>@<low 8 bits>', k = the order in which that exact address first appeared, so two runs of the same program
    give the same log unless the SEQUENCE of launches, a scalar argument, the aliasing pattern of the buffers or an alignment
    differs (tools/diff_traces.py compares two dumps).  A debugging aid: nothing in the product path sets it."""

    def __init__(self, inner):
        self._inner = inner
        self._ids: dict = {}

    def _norm(self, kind, v):
        if kind is _vp:
            if v is None:
                return "NULL"
            v = int(v)
            k = self._ids.setdefault(v, len(self._ids))
            return f"p{k}@{v & 0xFF:02x}"
        if isinstance(v, C.Array):                 # small by-pointer arrays (osk_rope_table's axes): their contents
            return tuple(int(x) for x in v)
        return round(float(v), 9) if kind in (_f32, _f64) else int(v)

    def __getattr__(self, name):
        fn = getattr(self._inner, name)
        sig = SIGNATURES.get(name)
        if sig is None:
            return fn

        def traced(*args):
            TRACE_LOG.append((name,) + tuple(self._norm(k, a) for k, a in zip(sig, args)))
            return fn(*args)

        return traced


TRACE_LOG: list = []
lib = _load()
if os.environ.get("OSK_TRACE"):
    lib = _TracingLib(lib)


OSK_EUNSUPPORTED = -2   # csrc/osk_common.h


def _check(status: int, what: str) -> None:
    if status != 0:
        kind = "invalid argument / unsupported shape" if status < 0 else "HIP error"
        raise RuntimeError(f"{what} failed: status {status} ({kind})")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t) -> int | None:
    return None if t is None else t.data_ptr()


# ----------------------------------------------------------------------------------------------
# thin wrappers (shape logic only)
# ----------------------------------------------------------------------------------------------
def ln_modulate(x: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, out: torch.Tensor,
                mod_batch_stride: int, eps: float = 1e-6) -> torch.Tensor:
    """x, out: bf16 [B, L, D] views with contiguous last dim; shift/scale f32 views whose row b starts at
    data_ptr + b*mod_batch_stride."""
    B, L, D = x.shape
    assert x.dtype == torch.bfloat16 and out.dtype == torch.bfloat16 and shift.dtype == torch.float32, (x.dtype, out.dtype)
    _check(lib.osk_ln_modulate_bf16(x.data_ptr(), x.stride(0), x.stride(1), out.data_ptr(), out.stride(0),
                                    out.stride(1), shift.data_ptr(), scale.data_ptr(), mod_batch_stride,
                                    B, L, D, eps, _stream()), "osk_ln_modulate_bf16")
    return out


# bench.py sets these to lists for a side measurement (never the timed region): (start, end, FLOPs) around every GEMM launch,
# (start, end) around every flash-attention launch
PROFILE_GEMM = None
PROFILE_ATTENTION = None


class _prof:
    """context: two HIP events around the launches inside, appended to `sink` (one of the lists above; None: off) with `extra`"""

    def __init__(self, sink, *extra):
        self.sink, self.extra = sink, extra

    def __enter__(self):
        if self.sink is not None:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if self.sink is not None:
            self.e1.record()
            self.sink.append((self.e0, self.e1, *self.extra))
        return False


def _gemm_prof(flops: float) -> _prof:
    return _prof(PROFILE_GEMM, flops)


def _attn_prof() -> _prof:
    return _prof(PROFILE_ATTENTION)


def gemm(a: torch.Tensor, w: torch.Tensor, bias, out: torch.Tensor, *, res=None, gate=None,
         gate_batch_stride: int = 0, gelu_from: int | None = None) -> torch.Tensor:
    """a bf16 [B, L, K] view (last dim contiguous), w bf16 [N, K] (row stride arbitrary), bias f32 [N] | None,
    out bf16/f32 [B, L, N] view.  res (bf16 view shaped like out, same strides) and gate (f32, row b at
    data_ptr + b*gate_batch_stride) select the gate*x + residual epilogue."""
    B, L, K = a.shape
    N = w.shape[0]
    assert out.shape[0] == B and out.shape[1] == L and out.shape[2] == N
    assert a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and out.dtype in (torch.bfloat16, torch.float32), \
        (a.dtype, w.dtype, out.dtype)
    if res is not None:
        assert res.stride() == out.stride() and res.dtype == torch.bfloat16
    with _gemm_prof(2.0 * B * L * N * K):
        _check(lib.osk_gemm_bf16(a.data_ptr(), a.stride(0), a.stride(1), L, w.data_ptr(), w.stride(0), _p(bias),
                                 out.data_ptr(), out.stride(0), out.stride(1), L, _p(res), _p(gate),
                                 gate_batch_stride, B * L, N, K, N if gelu_from is None else gelu_from,
                                 1 if out.dtype == torch.float32 else 0, _stream()), "osk_gemm_bf16")
    return out


def gemm_tile_kind(a: torch.Tensor, w: torch.Tensor) -> int:
    """the tile kernel gemm(a, w, ...) launches for these operands (osk_gemm_tile_choice_strided: the dispatch's own code, nothing is
    launched): 2 = 256 x 256, 1 = 256 x 128, 0 = 128 x 128.  a bf16 [B, L, K] view, w bf16 [N, K]; the views may span more than 4 GiB."""
    B, L, K = a.shape
    kind = lib.osk_gemm_tile_choice_strided(B * L, w.shape[0], K, a.stride(0), a.stride(1), L, w.stride(0))
    if kind < 0:
        _check(kind, "osk_gemm_tile_choice_strided")
    return kind


def geglu_pack(w_value: torch.Tensor, w_gate: torch.Tensor, b_value=None, b_gate=None):
    """Weights of a GEGLU up-projection in the row order osk_gemm_geglu_bf16 wants: value and gate rows interleaved in blocks of 16
    (include/osk.h).  w_* [N_out, K] -> [2 N_out, K]; biases f32 [N_out] -> [2 N_out] (or None).  Done once, at plan time."""
    n, k = w_value.shape
    assert w_gate.shape == (n, k) and n % 16 == 0
    w = torch.stack((w_value.reshape(n // 16, 16, k), w_gate.reshape(n // 16, 16, k)), 1).reshape(2 * n, k).contiguous()
    b = None
    if b_value is not None:
        b = torch.stack((b_value.float().reshape(n // 16, 16), b_gate.float().reshape(n // 16, 16)), 1).reshape(2 * n).contiguous()
    return w, b


def gemm_geglu(a: torch.Tensor, w_packed: torch.Tensor, bias_packed, out: torch.Tensor, workspace: torch.Tensor | None = None):
    """out[b, l, j] = value * gelu_tanh(gate) of the packed projection (geglu_pack); a bf16 [B, L, K], out bf16 [B, L, N_out].
    workspace (uint8 / bf16, >= B L 2 N_out 2 bytes): only shapes off the 256 x 256 tile path need it."""
    B, L, K = a.shape
    n_out = w_packed.shape[0] // 2
    assert out.shape == (B, L, n_out) and a.dtype == out.dtype == w_packed.dtype == torch.bfloat16
    _check(lib.osk_gemm_geglu_bf16(a.data_ptr(), a.stride(0), a.stride(1), L, w_packed.data_ptr(), w_packed.stride(0), _p(bias_packed),
                                   out.data_ptr(), out.stride(0), out.stride(1), L, B * L, n_out, K, _p(workspace),
                                   0 if workspace is None else workspace.numel() * workspace.element_size(), _stream()),
           "osk_gemm_geglu_bf16")
    return out


class OskGemmOperands(C.Structure):
    """include/osk.h::OskGemmOperands"""
    _fields_ = [("A", _vp), ("a_batch_stride", _i64), ("a_row_stride", _i64), ("a_rows_per_batch", _i32),
                ("W", _vp), ("w_row_stride", _i64), ("bias", _vp),
                ("C", _vp), ("c_batch_stride", _i64), ("c_row_stride", _i64), ("c_rows_per_batch", _i32),
                ("res", _vp), ("gate", _vp), ("gate_batch_stride", _i64), ("M", _i32)]


def _gemm_operands(a, w, bias, out, res, gate, gate_batch_stride, *, wide_out: bool = False) -> OskGemmOperands:
    """wide_out: the output tensor may be WIDER than the task's N (a skip range / a column slice of gemm_group: the row layout
    [q | k | . | mlp] is addressed through its row stride)"""
    B, L, K = a.shape
    assert out.shape[0] == B and out.shape[1] == L and (out.shape[2] >= 1 if wide_out else out.shape[2] == w.shape[0]) and w.shape[1] == K
    assert a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and out.dtype == torch.bfloat16
    if res is not None:
        assert res.stride() == out.stride() and res.dtype == torch.bfloat16
    return OskGemmOperands(a.data_ptr(), a.stride(0), a.stride(1), L, w.data_ptr(), w.stride(0), _p(bias), out.data_ptr(),
                           out.stride(0), out.stride(1), L, _p(res), _p(gate), gate_batch_stride, B * L)


def gemm_pair(first: dict, second: dict, *, gelu_from: int | None = None) -> None:
    """two gemm() calls that share N, K and the epilogue kind in one launch (osk_gemm_bf16_pair): each dict holds gemm()'s
    arguments a, w, bias, out and optionally res, gate, gate_batch_stride.  The img- / txt-stream Linear pairs of a double block."""
    ops = [_gemm_operands(d["a"], d["w"], d["bias"], d["out"], d.get("res"), d.get("gate"), d.get("gate_batch_stride", 0))
           for d in (first, second)]
    N, K = first["w"].shape
    assert tuple(second["w"].shape) == (N, K)
    with _gemm_prof(2.0 * (ops[0].M + ops[1].M) * N * K):
        _check(lib.osk_gemm_bf16_pair(C.addressof(ops[0]), C.addressof(ops[1]), N, K, N if gelu_from is None else gelu_from,
                                      _stream()), "osk_gemm_bf16_pair")


class OskGemmTask(C.Structure):
    """include/osk.h::OskGemmTask"""
    _fields_ = [("op", OskGemmOperands), ("N", _i32), ("gelu_from", _i32), ("skip_from", _i32), ("skip_len", _i32), ("vt_head_dim", _i32)]


def gemm_group(tasks: list) -> bool:
    """osk_gemm_group_bf16: up to four problems sharing K in one launch.  Each task is a dict:
      plain:  a, w, bias, out [, res, gate, gate_batch_stride, gelu_from, skip=(from, len)]  -- gemm()'s arguments; with `skip` the
              physical columns [from, from + len) of w / bias / out are neither computed nor stored
      V^T:    x (bf16 [B, L, K] view), w (W_v [H*hd, K]), bias (f32 | None), vt (bf16 [B, H, hd, Lp] contiguous), vt_pos (first position on
              the key axis, % 64 == 0), hd
    Returns False -- nothing launched -- when the library declines the group (OSK_EUNSUPPORTED: a task off the 256 x 256 tile path);
    the caller then runs the single calls."""
    arr = (OskGemmTask * len(tasks))()
    K = None
    flops = 0.0
    for t, d in zip(arr, tasks):
        if "vt" in d:
            x, w, vt = d["x"], d["w"], d["vt"]
            B, L, k_ = x.shape
            assert x.dtype == w.dtype == vt.dtype == torch.bfloat16 and vt.is_contiguous() and vt.dim() == 4 and d["vt_pos"] % 64 == 0
            assert vt.shape[0] == B and vt.shape[1] * vt.shape[2] == w.shape[0] and d["vt_pos"] + (L + 63) // 64 * 64 <= vt.shape[3]
            t.op = OskGemmOperands(x.data_ptr(), x.stride(0), x.stride(1), L, w.data_ptr(), w.stride(0), _p(d.get("bias")),
                                   vt.data_ptr() + 2 * d["vt_pos"], vt.stride(0), vt.stride(2), L, None, None, 0, B * L)
            t.N, t.gelu_from, t.skip_from, t.skip_len, t.vt_head_dim = w.shape[0], w.shape[0], 0, 0, d["hd"]
            flops += 2.0 * B * L * w.shape[0] * k_
        else:
            a, w, out = d["a"], d["w"], d["out"]
            k_ = a.shape[2]
            t.op = _gemm_operands(a, w, d.get("bias"), out, d.get("res"), d.get("gate"), d.get("gate_batch_stride", 0), wide_out=True)
            sf, sl = d.get("skip", (0, 0))
            t.N, t.gelu_from, t.skip_from, t.skip_len, t.vt_head_dim = w.shape[0], d.get("gelu_from", w.shape[0]) if d.get("gelu_from") is not None else w.shape[0], sf, sl, 0
            flops += 2.0 * a.shape[0] * a.shape[1] * (w.shape[0] - sl) * k_
        assert K in (None, k_), "the tasks of a group share K"
        K = k_
    with _gemm_prof(flops):
        rc = lib.osk_gemm_group_bf16(C.addressof(arr), len(tasks), K, _stream())
    if rc == OSK_EUNSUPPORTED:
        return False
    _check(rc, "osk_gemm_group_bf16")
    return True


def ln_modulate_fp8(x: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, mod_batch_stride: int, eps: float = 1e-6):
    """ln_modulate + quantize_rows_fp8 in one pass: x bf16 [B, L, D] view -> (e4m3 bytes uint8 [B*L, D], f32 scales [B*L])."""
    B, L, D = x.shape
    out8 = torch.empty(B * L, D, dtype=torch.uint8, device=x.device)
    scales = torch.empty(B * L, dtype=torch.float32, device=x.device)
    _check(lib.osk_ln_modulate_fp8(x.data_ptr(), x.stride(0), x.stride(1), out8.data_ptr(), scales.data_ptr(),
                                   shift.data_ptr(), scale.data_ptr(), mod_batch_stride, B, L, D, eps, _stream()),
           "osk_ln_modulate_fp8")
    return out8, scales


def quantize_rows_fp8(x: torch.Tensor, out8: torch.Tensor | None = None, scales: torch.Tensor | None = None):
    """x bf16 [B, L, K] view (or [N, K] weight) -> (e4m3 bytes as uint8 [B*L, K] contiguous, f32 scales [B*L])."""
    if x.dim() == 2:
        x = x.unsqueeze(0)
    B, L, K = x.shape
    M = B * L
    if out8 is None:
        out8 = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    if scales is None:
        scales = torch.empty(M, dtype=torch.float32, device=x.device)
    assert out8.is_contiguous() and out8.numel() == M * K and scales.numel() >= M
    _check(lib.osk_quantize_rows_fp8(x.data_ptr(), x.stride(0), x.stride(1), L, out8.data_ptr(), scales.data_ptr(),
                                     M, K, _stream()), "osk_quantize_rows_fp8")
    return out8, scales


def gemm_fp8_supported(M: int, N: int, K: int) -> bool:
    """shapes the fp8 instantiation of the large-tile kernel takes (include/osk.h); others stay on gemm().
    Mirrors gemm256_fp8_supported (csrc/gemm256.hip) for the contiguous images the host passes: the kernel addresses every tile
    relative to its own origin, so what has to fit its 32-bit per-lane offsets is a 256-row window (256 K bytes), not the image --
    M * K and N * K may exceed 4 GiB."""
    return M >= 256 and N >= 128 and K % 128 == 0 and 256 * K <= 0xFFFFFFFF


def gemm_fp8(a8: torch.Tensor, a_scale: torch.Tensor, w8: torch.Tensor, w_scale: torch.Tensor, bias,
             out: torch.Tensor, *, res=None, gate=None, gate_batch_stride: int = 0,
             gelu_from: int | None = None) -> torch.Tensor:
    """a8 uint8 (e4m3) [M, K] contiguous with scales f32 [M]; w8 uint8 [N, K] with scales f32 [N]; out bf16/f32
    [B, L, N] view with B * L == M; epilogue arguments as gemm()."""
    M, K = a8.shape
    N = w8.shape[0]
    B, L = out.shape[0], out.shape[1]
    assert B * L == M and out.shape[2] == N and w8.shape[1] == K
    if res is not None:
        assert res.stride() == out.stride()
    with _gemm_prof(2.0 * M * N * K):
        _check(lib.osk_gemm_fp8(a8.data_ptr(), 0, a8.stride(0), M, a_scale.data_ptr(), w8.data_ptr(), w8.stride(0),
                                w_scale.data_ptr(), _p(bias), out.data_ptr(), out.stride(0), out.stride(1), L, _p(res),
                                _p(gate), gate_batch_stride, M, N, K, N if gelu_from is None else gelu_from,
                                1 if out.dtype == torch.float32 else 0, _stream()), "osk_gemm_fp8")
    return out


def gemv_tasks(x: torch.Tensor, tasks, out: torch.Tensor, act_in: int = 0, accumulate: bool = False):
    """tasks: GemvTasks (device descriptor arrays).  x f32 [Bv, K], out f32 [Bv, *]."""
    Bv, K = x.shape
    _check(lib.osk_gemv_tasks_bf16(x.data_ptr(), x.stride(0), Bv, K, tasks.w_ptrs.data_ptr(),
                                   tasks.b_ptrs.data_ptr(), tasks.out_cols.data_ptr(),
                                   tasks.n_rows.data_ptr(), tasks.n_tasks, out.data_ptr(), out.stride(0),
                                   act_in, 1 if accumulate else 0, _stream()), "osk_gemv_tasks_bf16")
    return out


class GemvTasks:
    """Device-side task list for osk_gemv_tasks_bf16: a list of (weight bf16 [N, K], bias bf16 [N] | None,
    out column offset); each layer is cut into tasks of <= 64 rows.  Keeps the tensors alive."""

    ROWS = 64

    def __init__(self, layers, device):
        wp, bp, oc, nr = [], [], [], []
        self._keep = []
        for w, b, col in layers:
            assert w.dtype == torch.bfloat16 and w.is_contiguous()
            self._keep.append((w, b))
            N, K = w.shape
            for r0 in range(0, N, self.ROWS):
                n = min(self.ROWS, N - r0)
                wp.append(w.data_ptr() + r0 * K * 2)
                bp.append(0 if b is None else b.data_ptr() + r0 * 2)
                oc.append(col + r0)
                nr.append(n)
        self.n_tasks = len(wp)
        # uint64 pointers stored bit-exactly in int64 tensors
        to_i64 = lambda v: v - (1 << 64) if v >= (1 << 63) else v
        self.w_ptrs = torch.tensor([to_i64(v) for v in wp], dtype=torch.int64, device=device)
        self.b_ptrs = torch.tensor([to_i64(v) for v in bp], dtype=torch.int64, device=device)
        self.out_cols = torch.tensor(oc, dtype=torch.int32, device=device)
        self.n_rows = torch.tensor(nr, dtype=torch.int32, device=device)


def timestep_embedding(t: torch.Tensor, out: torch.Tensor, max_period: float = 10000.0,
                       time_factor: float = 1000.0) -> torch.Tensor:
    B, dim = out.shape
    _check(lib.osk_timestep_embedding(t.data_ptr(), B, dim, max_period, time_factor, out.data_ptr(), _stream()),
           "osk_timestep_embedding")
    return out


def rope_table(ids: torch.Tensor, axes_dim, theta: float, f32_angles: bool, cos: torch.Tensor, sin: torch.Tensor):
    """ids f32 [n_rows, n_axes] contiguous -> cos/sin f32 [n_rows, sum(axes)/2]."""
    n_rows, n_axes = ids.shape
    arr = (_i32 * n_axes)(*[int(a) for a in axes_dim])
    _check(lib.osk_rope_table(ids.data_ptr(), n_rows, n_axes, arr, float(theta), 1 if f32_angles else 0,
                              cos.data_ptr(), sin.data_ptr(), _stream()), "osk_rope_table")


def qknorm_rope(q: torch.Tensor, k: torch.Tensor, qs0, ks0, qs1, ks1, l_split: int, cos, sin,
                cs_batch_stride: int, H: int, hd: int, rope_mode: int, eps: float = 1e-6, q_mult: float = 1.0):
    """q, k: bf16 [B, L, H*hd] views (same strides, last dim contiguous) rewritten in place; one of them may
    be None (one-sided call).  q_mult: factor folded into q before its final rounding (attention_fwd q_prescaled)."""
    t = q if q is not None else k
    B, L, _ = t.shape
    assert q is None or k is None or q.stride() == k.stride()
    _check(lib.osk_qknorm_rope_bf16(_p(q), _p(k), t.stride(0), t.stride(1), qs0.data_ptr(),
                                    ks0.data_ptr(), qs1.data_ptr(), ks1.data_ptr(), l_split, cos.data_ptr(),
                                    sin.data_ptr(), cs_batch_stride, B, L, H, hd, rope_mode, eps, q_mult, _stream()),
           "osk_qknorm_rope_bf16")


def v_transpose(v: torch.Tensor, vt: torch.Tensor, H: int, hd: int):
    """v bf16 [B, L, H*hd] view -> vt bf16 [B, H, hd, round_up(L, 64)] contiguous."""
    B, L, _ = v.shape
    _check(lib.osk_v_transpose_bf16(v.data_ptr(), v.stride(0), v.stride(1), vt.data_ptr(), B, L, H, hd, _stream()),
           "osk_v_transpose_bf16")


def kv_join(k_seg: torch.Tensor, v_seg: torch.Tensor, k_out: torch.Tensor, vt_out: torch.Tensor, H: int, hd: int, L: int):
    """k_seg, v_seg bf16 [n_seg, B, seg_len, H*hd] views with the same strides (the gathered exchange buffers: key j in segment
    j // seg_len, row j % seg_len) -> k_out bf16 [B, L, H*hd] view and vt_out bf16 [B, H, hd, round_up(L, 64)] contiguous, vt_out
    bit for bit v_transpose() of the L keys as one contiguous V (osk_kv_join_bf16).  (n_seg - 1) * seg_len < L <= n_seg * seg_len."""
    n_seg, B, seg_len, D = k_seg.shape
    assert k_seg.dtype == v_seg.dtype == k_out.dtype == vt_out.dtype == torch.bfloat16 and D == H * hd, (k_seg.dtype, v_seg.dtype, D, H, hd)
    assert v_seg.shape == k_seg.shape and v_seg.stride() == k_seg.stride() and k_seg.stride(3) == 1, (v_seg.shape, v_seg.stride(), k_seg.stride())
    assert tuple(k_out.shape) == (B, L, D) and k_out.stride(2) == 1, (k_out.shape, k_out.stride())
    assert tuple(vt_out.shape) == (B, H, hd, (L + 63) // 64 * 64) and vt_out.is_contiguous(), (vt_out.shape, vt_out.stride())
    _check(lib.osk_kv_join_bf16(k_seg.data_ptr(), v_seg.data_ptr(), k_seg.stride(0), k_seg.stride(1), k_seg.stride(2), k_out.data_ptr(),
                                k_out.stride(0), k_out.stride(1), vt_out.data_ptr(), B, H, hd, n_seg, seg_len, L, _stream()),
           "osk_kv_join_bf16")


_ATTN_WS: dict = {}


def attention_workspace(device) -> torch.Tensor:
    """workspace for the tail split of osk_attention_fwd_ws_bf16, one per (device, stream): launches are ordered within a
    stream (the merge kernel of one launch has consumed the buffer before the next launch writes it), not across
    streams.  Allocated once per key, reused by every launch."""
    dev = torch.device(device)
    key = (str(dev), torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0)
    ws = _ATTN_WS.get(key)
    if ws is None:
        ws = _ATTN_WS[key] = torch.empty(lib.osk_attention_workspace_bytes(), dtype=torch.uint8, device=dev)
    return ws


def _attn_call(name: str, q, k, vt, out, H, hd, scale, lse, n_seg, seg_len, k_seg_stride, vt_seg_stride, q_prescaled, kv_batches,
               workspace, own=(), after_vt=()):
    """the C call of the three flash-attention wrappers below (their arguments, in their order).  own: the entry point's arguments
    between kv_batches and the workspace; after_vt: those between the V^T stride and out."""
    B, Lq, _ = q.shape
    with _attn_prof():
        _check(getattr(lib, name)(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k_seg_stride, k.stride(0), k.stride(1),
                                  vt.data_ptr(), vt_seg_stride, *after_vt, out.data_ptr(), out.stride(0), out.stride(1), _p(lse),
                                  B, H, Lq, n_seg, k.shape[1] if seg_len is None else seg_len, hd, scale, int(q_prescaled),
                                  kv_batches, *own, _p(workspace), 0 if workspace is None else workspace.numel(), _stream()), name)
    return out


def attention_fwd(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, H: int, hd: int,
                  scale: float, *, lse=None, n_seg: int = 1, seg_len: int | None = None,
                  k_seg_stride: int = 0, vt_seg_stride: int = 0, q_prescaled: bool = False, kv_batches: int = 0,
                  workspace: torch.Tensor | None = None, score_bound: float = 0.0):
    """q bf16 [B, Lq, H*hd] view; k bf16 [B, seg_len, H*hd] view of segment 0 (further segments k_seg_stride
    elements apart); vt from v_transpose (per segment); out bf16 [B, Lq, H*hd] view.  workspace (uint8, from
    attention_workspace()): lets the library split the workgroups of the grid's last partial round along the keys.
    score_bound > 0: |q . k| (as the kernel sees the scores, log2 units) never exceeds it -- enables the fast body
    (include/osk.h, osk_attention_fwd_bounded_bf16)."""
    if CHECK_SCORE_BOUND and score_bound > 0 and not torch.cuda.is_current_stream_capturing():   # (the check syncs: illegal in a capture)
        _assert_score_bound(q, k, H, hd, scale, n_seg, k.shape[1] if seg_len is None else seg_len, k_seg_stride, q_prescaled, kv_batches,
                            score_bound)
    return _attn_call("osk_attention_fwd_bounded_bf16", q, k, vt, out, H, hd, scale, lse, n_seg, seg_len, k_seg_stride, vt_seg_stride,
                      q_prescaled, kv_batches, workspace, own=(float(score_bound),))


def rownorm2_max(x: torch.Tensor, out: torch.Tensor, H: int, hd: int, accumulate: bool = False) -> torch.Tensor:
    """out[b, h] = max_l |x[b, l, h, :]|^2 of a bf16 [B, L, H*hd] view (osk_rownorm2_max_bf16); out f32 [B, H] contiguous"""
    B, L, _ = x.shape
    assert x.dtype == torch.bfloat16 and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * H
    _check(lib.osk_rownorm2_max_bf16(x.data_ptr(), x.stride(0), x.stride(1), B, L, H, hd, out.data_ptr(), 1 if accumulate else 0, _stream()),
           "osk_rownorm2_max_bf16")
    return out


def attention_fwd_auto(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, H: int, hd: int, scale: float,
                       qn2: torch.Tensor, kn2: torch.Tensor, *, lse=None, n_seg: int = 1, seg_len: int | None = None,
                       k_seg_stride: int = 0, vt_seg_stride: int = 0, q_prescaled: bool = True, kv_batches: int = 0,
                       workspace: torch.Tensor | None = None):
    """attention_fwd with the score bound taken from the operands on the device (osk_attention_fwd_auto_bf16): qn2 / kn2 from
    rownorm2_max() of the q / k of THIS call (f32 [B, H] / [kv_batches or B, H]).  Units whose bound allows it run the FAST body."""
    B = q.shape[0]
    assert qn2.dtype == kn2.dtype == torch.float32 and qn2.numel() == B * H and kn2.numel() == (kv_batches or B) * H
    return _attn_call("osk_attention_fwd_auto_bf16", q, k, vt, out, H, hd, scale, lse, n_seg, seg_len, k_seg_stride, vt_seg_stride,
                      q_prescaled, kv_batches, workspace, own=(qn2.data_ptr(), kn2.data_ptr()))


def attention_merge(parts: torch.Tensor, lse: torch.Tensor, out: torch.Tensor, H: int, hd: int,
                    lse_out: torch.Tensor | None = None) -> torch.Tensor:
    """out = the S attention results `parts` over disjoint key sets, merged by their log-sum-exp (osk_attention_merge_bf16):
    parts bf16 [S, B, L, H*hd] view (last dim contiguous, the other strides its own), lse f32 [S, B, H, L] contiguous (what
    attention_fwd(..., lse=) wrote beside each part), out bf16 [B, L, H*hd] view, lse_out f32 [B, H, L] contiguous or None."""
    assert parts.dim() == 4 and lse.dim() == 4 and out.dim() == 3, (parts.shape, lse.shape, out.shape)
    S, B, L, D = parts.shape
    assert 1 <= S <= 8 and D == H * hd and hd % 8 == 0, (parts.shape, H, hd)
    assert parts.dtype == torch.bfloat16 and out.dtype == torch.bfloat16 and tuple(out.shape) == (B, L, D), (parts.dtype, out.dtype, out.shape)
    assert lse.dtype == torch.float32 and lse.is_contiguous() and tuple(lse.shape) == (S, B, H, L), (lse.dtype, lse.shape, lse.stride())
    for t in (parts, out):
        assert t.stride(-1) == 1 and all(st % 8 == 0 for st in t.stride()[:-1]) and t.data_ptr() % 16 == 0, (t.stride(), t.data_ptr() % 16)
    if lse_out is not None:
        assert lse_out.dtype == torch.float32 and lse_out.is_contiguous() and tuple(lse_out.shape) == (B, H, L), (lse_out.dtype, lse_out.shape)
    _check(lib.osk_attention_merge_bf16(parts.data_ptr(), parts.stride(0), parts.stride(1), parts.stride(2), lse.data_ptr(),
                                        out.data_ptr(), out.stride(0), out.stride(1), _p(lse_out), S, B, H, L, hd, _stream()),
           "osk_attention_merge_bf16")
    return out


def _grown_workspace(kind: str, need: int, device) -> torch.Tensor:
    """a uint8 buffer of at least `need` bytes, one per (kind, device, stream) like attention_workspace(); grows to the largest request"""
    dev = torch.device(device)
    key = (kind, str(dev), torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0)
    ws = _ATTN_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _ATTN_WS[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    return ws


def attention_ragged_workspace(B: int, H: int, Lq: int, hd: int, device) -> torch.Tensor:
    """workspace of attention_fwd_ragged for these query dimensions, one per (device, stream) like attention_workspace(): the f32
    partials of the last-segment launch, launch A's lse, and the tail-split room of a plain call.  Grows to the largest request."""
    return _grown_workspace("ragged", lib.osk_attention_ragged_workspace_bytes(B, H, Lq, hd), device)


def _attn_operands(mode: int, q, k, k_scale, vt, v_scale, out, lse, H: int, hd: int, kv_batches: int, Lk: int, k_seg_stride: int = 0,
                   vt_seg_stride: int = 0, vt_keys: int | None = None):
    """the operand facts attention_fwd_ragged, attention_fwd_qk8 and the two window wrappers share, by mode (0 bf16, 1 pv8, 2 qk8:
    OSK_ATTN_* of include/osk.h, ATTN_MODES): q / out bf16 [B, Lq, H*hd] views; k the bf16 [Bkv, Lk, H*hd] view or, in mode 2, the
    packed k8 [Bkv, H, Lp, 128] of a segment of Lk keys (byte strides); the mode's f32 [Bkv, H] scale vectors; vt bf16 / vt8 bytes
    (with vt_keys: [..., hd | vt8_rows(hd), vt_keys]); lse f32 [B, H, Lq] when given.  Returns K's (batch stride, row stride) as
    the C calls take them."""
    assert mode != 2 or hd == 128, f"the fp8 QK^T kernel exists for head_dim 128 only, not {hd}"
    assert q.dim() == 3 and q.shape[2] == H * hd, (q.shape, H, hd)
    assert q.dtype == torch.bfloat16 and out.dtype == torch.bfloat16 and q.stride(2) == 1 and out.stride(2) == 1, (q.dtype, out.dtype, q.stride(), out.stride())
    assert q.stride(0) % 8 == 0 and q.stride(1) % 8 == 0 and q.data_ptr() % 16 == 0, (q.stride(), q.data_ptr() % 16)
    B, Lq, _ = q.shape
    Bkv = kv_batches or B
    for s_ in ((), (v_scale,), (k_scale, v_scale))[mode]:
        assert s_ is not None and s_.dtype == torch.float32 and s_.is_contiguous() and s_.numel() == Bkv * H, "scales: f32 [Bkv, H]"
    if mode == 2:
        assert k.dtype == torch.uint8 and k.dim() == 4 and k.stride(3) == 1 and k.stride(2) == 128, (k.dtype, k.shape, k.stride())
        assert tuple(k.shape) == k8_shape(Bkv, H, Lk, hd) and k.stride(1) == k.shape[2] * 128, (k.shape, k.stride(), Lk)
        assert k.data_ptr() % 16 == 0 and k.stride(0) % 16 == 0 and k_seg_stride % 16 == 0, (k.stride(), k_seg_stride)
    else:
        assert k.dtype == torch.bfloat16 and k.dim() == 3 and k.stride(2) == 1 and k.shape[2] == H * hd, (k.dtype, k.shape, k.stride())
        assert k.stride(0) % 8 == 0 and k.stride(1) % 8 == 0 and k_seg_stride % 8 == 0 and k.data_ptr() % 16 == 0, (k.stride(), k_seg_stride)
    assert vt.dtype == (torch.bfloat16 if mode == 0 else torch.uint8) and vt.data_ptr() % 16 == 0, (vt.dtype, vt.data_ptr() % 16)
    assert vt_seg_stride % (8 if mode == 0 else 16) == 0, vt_seg_stride
    if vt_keys is not None:
        assert vt.shape[-2] == (hd if mode == 0 else vt8_rows(hd)) and vt.shape[-1] == vt_keys, (vt.shape, hd, vt_keys)
    if lse is not None:
        assert lse.dtype == torch.float32 and lse.is_contiguous() and tuple(lse.shape) == (B, H, Lq), (lse.dtype, lse.shape)
    return k.stride(0), 128 if mode == 2 else k.stride(1)


def attention_fwd_ragged(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, H: int, hd: int, scale: float, *,
                         n_seg: int, seg_len: int, last_seg_len: int, k_seg_stride: int, vt_seg_stride: int, workspace: torch.Tensor,
                         lse=None, q_prescaled: bool = False, kv_batches: int = 0, score_bound: float = 0.0,
                         k_scale: torch.Tensor | None = None, v_scale: torch.Tensor | None = None):
    """attention over n_seg key segments of seg_len keys whose LAST holds last_seg_len <= seg_len (osk_attention_fwd_ragged_bf16):
    one launch over the full segments, one over the last, one in-place merge.  Operands by the scales given: neither = bf16 (k, vt,
    score_bound as attention_fwd), v_scale = pv8 (vt = vt8, byte stride, as attention_fwd_pv8), k_scale too = qk8 (k = segment 0's
    k8 [Bkv, H, Lp, 128], byte stride, as attention_fwd_qk8).  The last segment lies n_seg - 1 segment strides in, laid out as a
    tensor of last_seg_len keys of its own (v_transpose / v_transpose_fp8 / k_pack_fp8 of those keys alone).  workspace: from
    attention_ragged_workspace()."""
    assert out.dim() == 3 and q.shape == out.shape, (q.shape, out.shape)
    assert n_seg >= 2 and 1 <= last_seg_len <= seg_len, (n_seg, seg_len, last_seg_len)
    assert out.stride(0) % 8 == 0 and out.stride(1) % 8 == 0 and out.data_ptr() % 16 == 0, (out.stride(), out.data_ptr() % 16)
    assert k_scale is None or v_scale is not None, "qk8 operands come with both scale vectors"
    mode = 0 if v_scale is None else (1 if k_scale is None else 2)
    kbs, krs = _attn_operands(mode, q, k, k_scale, vt, v_scale, out, lse, H, hd, kv_batches, seg_len, k_seg_stride, vt_seg_stride)
    B, Lq, _ = q.shape
    Bkv = kv_batches or B
    assert workspace is not None and workspace.dtype == torch.uint8 and workspace.data_ptr() % 16 == 0
    if CHECK_SCORE_BOUND and mode == 0 and score_bound > 0 and not torch.cuda.is_current_stream_capturing():
        _assert_score_bound(q, k, H, hd, scale, n_seg - 1, seg_len, k_seg_stride, q_prescaled, kv_batches, score_bound)
        k_last = torch.as_strided(k, (Bkv, last_seg_len, H * hd), k.stride(), k.storage_offset() + (n_seg - 1) * k_seg_stride)
        _assert_score_bound(q, k_last, H, hd, scale, 1, last_seg_len, 0, q_prescaled, kv_batches, score_bound)   # launch B's keys
    with _attn_prof():
        _check(lib.osk_attention_fwd_ragged_bf16(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k_seg_stride, kbs, krs, _p(k_scale),
                                                 vt.data_ptr(), vt_seg_stride, _p(v_scale), out.data_ptr(), out.stride(0), out.stride(1),
                                                 _p(lse), B, H, Lq, n_seg, seg_len, last_seg_len, hd, scale, int(q_prescaled), kv_batches,
                                                 float(score_bound), mode, workspace.data_ptr(), workspace.numel(), _stream()),
               "osk_attention_fwd_ragged_bf16")
    return out


def attention_window_workspace_bytes(B: int, H: int, Lq: int, hd: int) -> int:
    """bytes attention_fwd_window needs for these query dimensions (a caller that keeps a buffer of its own: mmdit's workspaces)"""
    return int(lib.osk_attention_window_workspace_bytes(B, H, Lq, hd))


def attention_window_workspace(B: int, H: int, Lq: int, hd: int, device) -> torch.Tensor:
    """workspace of attention_fwd_window for these query dimensions, one per (device, stream) like attention_workspace(): the f32
    partials of the prefix launch and launch A's lse.  Grows to the largest request."""
    return _grown_workspace("window", lib.osk_attention_window_workspace_bytes(B, H, Lq, hd), device)


def check_window_table(windows: torch.Tensor, Lq: int, Lk: int, n_prefix: int, n_suffix: int = 0) -> None:
    """ValueError unless `windows` is a host int32 [ceil(Lq / 256), 2] table of (first tile, tile count) whose every row lies
    inside the ceil((Lk - n_suffix - n_prefix) / 64) tiles of the body.  (The kernel clamps what it reads; a table it would have to
    clamp is a host bug and is refused here.)  n_suffix > 0 (attention_fwd_window_anchor): Lk - n_suffix a multiple of 64 beyond n_prefix."""
    if not (isinstance(windows, torch.Tensor) and windows.device.type == "cpu" and windows.dtype == torch.int32):
        raise ValueError("windows: a host (CPU) int32 tensor is expected")
    if n_prefix < 0 or n_prefix % 64 or n_prefix >= Lk:
        raise ValueError(f"n_prefix = {n_prefix}: a multiple of 64 in [0, Lk = {Lk}) is expected")
    if n_suffix < 0 or (n_suffix > 0 and ((Lk - n_suffix) % 64 or Lk - n_suffix <= n_prefix)):
        raise ValueError(f"n_suffix = {n_suffix}: 0, or Lk - n_suffix a multiple of 64 greater than n_prefix = {n_prefix} is expected (Lk = {Lk})")
    nqb, tiles = (Lq + 255) // 256, (Lk - n_suffix - n_prefix + 63) // 64
    if windows.dim() != 2 or tuple(windows.shape) != (nqb, 2):
        raise ValueError(f"windows: shape {tuple(windows.shape)}, expected ({nqb}, 2) = one row per 256 query rows")
    first, n = windows[:, 0], windows[:, 1]
    if bool((first < 0).any()):
        raise ValueError("windows: a negative first tile")
    if bool((n < 1).any()):
        raise ValueError("windows: an empty range (tile count < 1)")
    if bool((first.long() + n.long() > tiles).any()):
        raise ValueError(f"windows: a range ends past the body's {tiles} tiles")


_WINDOW_DEV: dict = {}


def _window_on_device(windows: torch.Tensor, device) -> torch.Tensor:
    """the device copy of a validated host table, uploaded once per (content, device) and kept: a call inside a captured region
    finds it here (upload the table by one call outside the capture first -- MMDiTModel does)."""
    c = windows.contiguous()
    key = (str(torch.device(device)), tuple(c.shape), c.numpy().tobytes())
    dev = _WINDOW_DEV.get(key)
    if dev is None:
        if torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("attention_fwd_window: this table was never uploaded; call once outside the captured region first")
        while len(_WINDOW_DEV) >= 64:    # (head-exchange sequence parallelism keeps one table per source rank and geometry)
            _WINDOW_DEV.pop(next(iter(_WINDOW_DEV)))
        dev = _WINDOW_DEV[key] = c.to(device)
    return dev


def _attention_window(mode: int, q, k, k_scale, vt, v_scale, out, H, hd, scale, n_prefix, windows, lse, q_prescaled, kv_batches, score_bound,
                      workspace, Lk, n_suffix=None):
    """the body of attention_fwd_window (mode 0) and attention_fwd_window_fp8 (modes 1, 2): checks, table upload, the C call of the mode.
    n_suffix (an int, 0 included): attention_fwd_window_anchor -- the same checks, the anchored entry with the mode as an argument"""
    assert out.dim() == 3 and q.shape == out.shape, (q.shape, out.shape)
    if mode == 2:
        assert Lk is not None and vt.dim() == 4, f"qk8: Lk = the key count (k8 only shows Lp = {k.shape[2]}); got {Lk}"
    else:
        assert Lk is None or Lk == k.shape[1], (Lk, k.shape)
        Lk = k.shape[1]
    Lp = (Lk + 63) // 64 * 64
    kbs, krs = _attn_operands(mode, q, k, k_scale, vt, v_scale, out, lse, H, hd, kv_batches, Lk, vt_keys=Lp)
    B, Lq, _ = q.shape
    check_window_table(windows, Lq, Lk, n_prefix, n_suffix or 0)
    assert vt.is_contiguous(), vt.stride()
    if n_suffix is not None and workspace is None:
        workspace = attention_window_anchor_workspace(B, H, Lq, hd, q.device)
    if n_prefix > 0 and workspace is None:
        workspace = attention_window_workspace(B, H, Lq, hd, q.device)
    win = _window_on_device(windows, q.device)
    if CHECK_SCORE_BOUND and mode == 0 and score_bound > 0 and not torch.cuda.is_current_stream_capturing():
        _assert_score_bound(q, k, H, hd, scale, 1, Lk, 0, q_prescaled, kv_batches, score_bound)
    if n_suffix is not None:
        with _attn_prof():
            _check(lib.osk_attention_fwd_window_anchor_bf16(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), kbs, krs, _p(k_scale),
                                                            vt.data_ptr(), _p(v_scale), out.data_ptr(), out.stride(0), out.stride(1),
                                                            _p(lse), B, H, Lq, Lk, n_prefix, int(n_suffix), hd, scale, int(q_prescaled),
                                                            kv_batches, float(score_bound), mode, win.data_ptr(), win.shape[0],
                                                            workspace.data_ptr(), workspace.numel(), _stream()),
                   "osk_attention_fwd_window_anchor_bf16")
        return out
    name = "osk_attention_fwd_window_bf16" if mode == 0 else "osk_attention_fwd_window_fp8_bf16"
    own = (float(score_bound),) if mode == 0 else (mode,)          # the argument between kv_batches and the table
    fp8 = ((_p(k_scale),), (v_scale.data_ptr(),)) if mode else ((), ())   # the scale vectors behind K's strides and behind V^T
    with _attn_prof():
        _check(getattr(lib, name)(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), kbs, krs, *fp8[0], vt.data_ptr(), *fp8[1],
                                  out.data_ptr(), out.stride(0), out.stride(1), _p(lse), B, H, Lq, Lk, n_prefix, hd, scale,
                                  int(q_prescaled), kv_batches, *own, win.data_ptr(), win.shape[0], _p(workspace),
                                  0 if workspace is None else workspace.numel(), _stream()), name)
    return out


def attention_fwd_window(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, H: int, hd: int, scale: float, *,
                         n_prefix: int, windows: torch.Tensor, lse=None, q_prescaled: bool = False, kv_batches: int = 0,
                         score_bound: float = 0.0, workspace: torch.Tensor | None = None):
    """attention in which the 256-row query block i sees keys [0, n_prefix) and the 64-key tiles windows[i] = (first, count) of the
    body keys [n_prefix, Lk), nothing else (osk_attention_fwd_window_bf16).  q, k, vt, out, lse, score_bound as attention_fwd with
    one key segment: k bf16 [Bkv, Lk, H*hd] view, vt = v_transpose of all Lk keys.  windows: HOST int32 [ceil(Lq / 256), 2],
    validated here (ValueError) and uploaded once per content.  workspace: from attention_window_workspace(); needed when
    n_prefix > 0 (taken from there when None)."""
    return _attention_window(0, q, k, None, vt, None, out, H, hd, scale, n_prefix, windows, lse, q_prescaled, kv_batches, score_bound,
                             workspace, None)


def attention_window_anchor_workspace_bytes(B: int, H: int, Lq: int, hd: int) -> int:
    """bytes attention_fwd_window_anchor needs for these query dimensions: two partial sets and launch A's lse"""
    return int(lib.osk_attention_window_anchor_workspace_bytes(B, H, Lq, hd))


def attention_window_anchor_workspace(B: int, H: int, Lq: int, hd: int, device) -> torch.Tensor:
    """workspace of attention_fwd_window_anchor for these query dimensions, one per (device, stream); grows to the largest request"""
    return _grown_workspace("window_anchor", lib.osk_attention_window_anchor_workspace_bytes(B, H, Lq, hd), device)


def attention_fwd_window_anchor(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, H: int, hd: int, scale: float, *,
                                n_prefix: int, n_suffix: int, windows: torch.Tensor, mode: str = "bf16", k_scale: torch.Tensor | None = None,
                                v_scale: torch.Tensor | None = None, lse=None, q_prescaled: bool = False, kv_batches: int = 0,
                                score_bound: float = 0.0, workspace: torch.Tensor | None = None, Lk: int | None = None):
    """frame-window attention with always-attended keys at BOTH ends (osk_attention_fwd_window_anchor_bf16): every query sees keys
    [0, n_prefix) and [Lk - n_suffix, Lk); the 256-row query block i sees, of the body keys between them, the 64-key tiles
    windows[i] = (first, count) and nothing else.  mode "bf16" (k, vt, score_bound as attention_fwd_window), "pv8" (vt = vt8 with
    v_scale) or "qk8" (k = k8 with k_scale too, Lk given), the operands of attention_fwd_window_fp8.  n_suffix = 0 is the window
    entry of that mode.  windows: HOST int32 [ceil(Lq / 256), 2] over the body's tiles, validated here.  workspace: from
    attention_window_anchor_workspace() (taken from there when None)."""
    if mode != "bf16" and mode not in ATTN_MODES:
        raise ValueError(f"attention_fwd_window_anchor: mode {mode!r}, expected 'bf16', 'pv8' or 'qk8'")
    m = 0 if mode == "bf16" else ATTN_MODES[mode]
    return _attention_window(m, q, k, k_scale if m == 2 else None, vt, v_scale if m else None, out, H, hd, scale, n_prefix, windows, lse,
                             q_prescaled, kv_batches, score_bound if m == 0 else 0.0, workspace, Lk, n_suffix=int(n_suffix))


def attention_merge_into2(out: torch.Tensor, lse: torch.Tensor, o_b: torch.Tensor, lse_b: torch.Tensor, o_c: torch.Tensor,
                          lse_c: torch.Tensor, H: int, hd: int) -> torch.Tensor:
    """fold TWO further attention results over other keys into (out, lse) in place, in one pass and with one rounding
    (osk_attention_merge_into2_bf16): the arguments of attention_merge_into with a second partial (o_c, lse_c) laid out as (o_b, lse_b)."""
    assert out.dim() == 3 and out.dtype == torch.bfloat16 and out.shape[2] == H * hd and out.stride(2) == 1, (out.shape, out.dtype, out.stride())
    B, Lq, _ = out.shape
    Lqp = (Lq + 255) // 256 * 256
    assert out.stride(0) % 8 == 0 and out.stride(1) % 8 == 0 and out.data_ptr() % 16 == 0, (out.stride(), out.data_ptr() % 16)
    assert lse.dtype == torch.float32 and lse.is_contiguous() and tuple(lse.shape) == (B, H, Lq), (lse.dtype, lse.shape)
    for o_, l_ in ((o_b, lse_b), (o_c, lse_c)):
        assert o_.dtype == torch.float32 and o_.is_contiguous() and tuple(o_.shape) == (B, H, Lqp, hd) and o_.data_ptr() % 16 == 0, (o_.dtype, o_.shape)
        assert l_.dtype == torch.float32 and l_.is_contiguous() and tuple(l_.shape) == (B, H, Lqp), (l_.dtype, l_.shape)
    _check(lib.osk_attention_merge_into2_bf16(out.data_ptr(), out.stride(0), out.stride(1), lse.data_ptr(), o_b.data_ptr(), lse_b.data_ptr(),
                                              o_c.data_ptr(), lse_c.data_ptr(), B, H, Lq, hd, _stream()), "osk_attention_merge_into2_bf16")
    return out


def attention_merge_into(out: torch.Tensor, lse: torch.Tensor, o_b: torch.Tensor, lse_b: torch.Tensor, H: int, hd: int) -> torch.Tensor:
    """fold a second attention result over other keys into (out, lse) in place (osk_attention_merge_into_bf16): out bf16 [B, Lq, H*hd]
    view, lse f32 [B, H, Lq]; o_b f32 [B, H, Lqp, hd] and lse_b f32 [B, H, Lqp] contiguous, Lqp = Lq rounded up to 256."""
    assert out.dim() == 3 and out.dtype == torch.bfloat16 and out.shape[2] == H * hd and out.stride(2) == 1, (out.shape, out.dtype, out.stride())
    B, Lq, _ = out.shape
    Lqp = (Lq + 255) // 256 * 256
    assert out.stride(0) % 8 == 0 and out.stride(1) % 8 == 0 and out.data_ptr() % 16 == 0, (out.stride(), out.data_ptr() % 16)
    assert lse.dtype == torch.float32 and lse.is_contiguous() and tuple(lse.shape) == (B, H, Lq), (lse.dtype, lse.shape)
    assert o_b.dtype == torch.float32 and o_b.is_contiguous() and tuple(o_b.shape) == (B, H, Lqp, hd) and o_b.data_ptr() % 16 == 0, (o_b.dtype, o_b.shape)
    assert lse_b.dtype == torch.float32 and lse_b.is_contiguous() and tuple(lse_b.shape) == (B, H, Lqp), (lse_b.dtype, lse_b.shape)
    _check(lib.osk_attention_merge_into_bf16(out.data_ptr(), out.stride(0), out.stride(1), lse.data_ptr(), o_b.data_ptr(), lse_b.data_ptr(),
                                             B, H, Lq, hd, _stream()), "osk_attention_merge_into_bf16")
    return out


def attention_short(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, H: int, hd: int, scale: float,
                    alibi_slopes: torch.Tensor | None = None) -> torch.Tensor:
    """softmax(scale q k^T - slope_h |i + Lk - Lq - j|) v for sequences of at most 64 tokens (osk_attention_short_bf16: the
    temporal-attention call shape); q [B, Lq, H*hd], k / v [B, Lk, H*hd] bf16 views, alibi_slopes f32 [H] or None."""
    B, Lq, _ = q.shape
    Lk = k.shape[1]
    if alibi_slopes is not None:
        assert alibi_slopes.dtype == torch.float32 and alibi_slopes.is_contiguous() and alibi_slopes.numel() == H
    _check(lib.osk_attention_short_bf16(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1), v.data_ptr(),
                                        v.stride(0), v.stride(1), out.data_ptr(), out.stride(0), out.stride(1), _p(alibi_slopes),
                                        B, H, Lq, Lk, hd, scale, _stream()), "osk_attention_short_bf16")
    return out


def attention_relbias(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, H: int, hd: int, scale: float,
                      bias: torch.Tensor | None = None) -> torch.Tensor:
    """softmax(scale q k^T + bias[h, (j - i) + L - 1]) v, the T5 self-attention (osk_attention_relbias_bf16); q, k, v, out bf16
    [B, L, H*hd] views with contiguous last dim (q, k, v may be column groups of one fused projection output); bias f32
    [H, >= 2L - 1] with contiguous rows (any row stride) or None."""
    B, L, C = q.shape
    assert C == H * hd and k.shape == q.shape and v.shape == q.shape and out.shape == q.shape, (q.shape, k.shape, v.shape, out.shape)
    assert q.dtype == k.dtype == v.dtype == out.dtype == torch.bfloat16, (q.dtype, k.dtype, v.dtype, out.dtype)
    for t in (q, k, v):
        assert t.stride(2) == 1 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and t.data_ptr() % 16 == 0, (t.stride(), t.data_ptr() % 16)
    assert out.stride(2) == 1 and out.stride(0) % 4 == 0 and out.stride(1) % 4 == 0 and out.data_ptr() % 8 == 0, out.stride()
    brs = 0
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.dim() == 2 and bias.shape[0] == H and bias.shape[1] >= 2 * L - 1, (bias.dtype, bias.shape)
        assert bias.stride(1) == 1 and bias.stride(0) >= 2 * L - 1, bias.stride()
        brs = bias.stride(0)
    _check(lib.osk_attention_relbias_bf16(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1), v.data_ptr(),
                                          v.stride(0), v.stride(1), out.data_ptr(), out.stride(0), out.stride(1), _p(bias), brs,
                                          B, H, L, hd, scale, _stream()), "osk_attention_relbias_bf16")
    return out


def attention_launch_shape(B: int, H: int, Lq: int, n_seg: int, seg_len: int, hd: int, score_bound: float, workspace_bytes: int):
    """(key parts of the last round's work units, query rows per work unit) of a bounded attention call with these arguments"""
    rows = _i32(0)
    parts = lib.osk_attention_launch_shape(B, H, Lq, n_seg, seg_len, hd, float(score_bound), int(workspace_bytes), C.byref(rows))
    return int(parts), int(rows.value)


def attention_body(hd: int, n_seg: int, seg_len: int, score_bound: float) -> str:
    """which loop body attention_fwd(..., score_bound=...) runs for this key layout (reporting: bench.py, tests)"""
    return lib.osk_attention_body_name(hd, n_seg, seg_len, float(score_bound)).decode()


# OSK_CHECK_SCORE_BOUND=1 (debugging runs; its own switch since round 5 -- the call tracer OSK_TRACE only records calls, as its
# docstring says): every bounded attention call checks the caller's promise on the device before it launches -- the bounded loop
# body has no running maximum, so a violated bound silently loses accuracy (or, far beyond it, overflows).  The check is the
# sufficient condition the model's own bound is derived from (Cauchy-Schwarz per head): max |q_h| * max |k_h| <= bound.  It reads a
# device scalar back (a blocking sync), so it is skipped while the stream is being captured into a hipGraph.
CHECK_SCORE_BOUND = bool(os.environ.get("OSK_CHECK_SCORE_BOUND"))


def _assert_score_bound(q, k, H, hd, scale, n_seg, seg_len, k_seg_stride, q_prescaled, kv_batches, bound):
    Bq, Lq, _ = q.shape
    Bk = kv_batches if kv_batches else Bq
    qn = q.float().reshape(Bq, Lq, H, hd).norm(dim=-1).amax()
    if not q_prescaled:
        qn = qn * (scale * 1.4426950408889634)
    kn = torch.zeros((), dtype=torch.float32, device=q.device)
    for s_ in range(n_seg):
        ks = torch.as_strided(k, (Bk, seg_len, H * hd), (k.stride(0), k.stride(1), 1), k.storage_offset() + s_ * k_seg_stride)
        kn = torch.maximum(kn, ks.float().reshape(Bk, seg_len, H, hd).norm(dim=-1).amax())
    worst = float(qn * kn)
    if worst > bound * (1 + 2.0 ** -7):
        raise RuntimeError(f"osk_attention_fwd_bounded_bf16: the caller's score bound {bound:.4g} does not hold: max |q| max |k| = {worst:.4g} "
                           "(log2 units) -- the QK-norm scale vectors changed after the plan was built?")


def vt8_rows(hd: int) -> int:
    """rows per head of the e4m3 V^T tensor: hd dims + the ones row, rounded up to 16"""
    return (hd + 1 + 15) // 16 * 16


def v_scale_fp8(v: torch.Tensor, H: int, hd: int) -> torch.Tensor:
    """v bf16 [B, L, H*hd] view -> e4m3 scales f32 [B, H] = absmax per (batch, head) / 448"""
    B, L, _ = v.shape
    scales = torch.empty(B, H, dtype=torch.float32, device=v.device)
    _check(lib.osk_v_scale_fp8(v.data_ptr(), v.stride(0), v.stride(1), scales.data_ptr(), B, L, H, hd, _stream()),
           "osk_v_scale_fp8")
    return scales


def kv_scale_fp8(k: torch.Tensor, v: torch.Tensor, H: int, hd: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """k, v bf16 [B, L, H*hd] views (their own strides) -> f32 [2, B, H]: [0] = v_scale_fp8(k), [1] = v_scale_fp8(v), bit for bit,
    from one launch into one contiguous buffer (osk_kv_scale_fp8) -- what sequence parallelism max-reduces with ONE collective."""
    assert k.dim() == 3 and k.shape == v.shape, (k.shape, v.shape)
    B, L, C_ = k.shape
    assert k.dtype == torch.bfloat16 and v.dtype == torch.bfloat16 and C_ == H * hd and hd % 8 == 0, (k.dtype, v.dtype, k.shape, H, hd)
    for t in (k, v):
        assert t.stride(2) == 1 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and t.data_ptr() % 16 == 0, (t.stride(), t.data_ptr() % 16)
    if out is None:
        out = torch.empty(2, B, H, dtype=torch.float32, device=k.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (2, B, H) and out.device == k.device, (out.dtype, out.shape)
    _check(lib.osk_kv_scale_fp8(k.data_ptr(), k.stride(0), k.stride(1), v.data_ptr(), v.stride(0), v.stride(1), out.data_ptr(),
                                B, L, H, hd, _stream()), "osk_kv_scale_fp8")
    return out


def v_transpose_fp8(v: torch.Tensor, scales: torch.Tensor, vt8: torch.Tensor, H: int, hd: int) -> torch.Tensor:
    """v bf16 [B, L, H*hd] view, scales f32 [B, H] -> vt8 uint8 [B, H, vt8_rows(hd), Lp] (e4m3 bytes, kernel key order)."""
    B, L, _ = v.shape
    assert vt8.dtype == torch.uint8 and vt8.is_contiguous() and vt8.shape[-2] == vt8_rows(hd)
    assert scales.dtype == torch.float32 and scales.is_contiguous() and scales.numel() == B * H
    _check(lib.osk_v_transpose_fp8(v.data_ptr(), v.stride(0), v.stride(1), scales.data_ptr(), vt8.data_ptr(), B, L, H, hd,
                                   _stream()), "osk_v_transpose_fp8")
    return vt8


def attention_fwd_pv8(q: torch.Tensor, k: torch.Tensor, vt8: torch.Tensor, v_scale: torch.Tensor, out: torch.Tensor,
                      H: int, hd: int, scale: float, *, lse=None, n_seg: int = 1, seg_len: int | None = None,
                      k_seg_stride: int = 0, vt_seg_stride: int = 0, q_prescaled: bool = False, kv_batches: int = 0,
                      workspace: torch.Tensor | None = None):
    """attention_fwd with the P.V product on the fp8 MFMA: vt8 / v_scale from v_transpose_fp8 (vt_seg_stride in bytes)."""
    return _attn_call("osk_attention_fwd_pv8_bf16", q, k, vt8, out, H, hd, scale, lse, n_seg, seg_len, k_seg_stride, vt_seg_stride,
                      q_prescaled, kv_batches, workspace, after_vt=(v_scale.data_ptr(),))


def k8_shape(B: int, H: int, L: int, hd: int = 128) -> tuple:
    """shape of the e4m3 K tensor of one key segment of L keys: [B, H, L rounded up to 64, 128] (head_dim 128 only)"""
    assert hd == 128, f"the fp8 QK^T kernel exists for head_dim 128 only, not {hd}"
    return (B, H, (L + 63) // 64 * 64, 128)


def k_pack_fp8(k: torch.Tensor, scales: torch.Tensor, k8: torch.Tensor, H: int, hd: int) -> torch.Tensor:
    """k bf16 [B, L, H*128] view, scales f32 [B, H] (v_scale_fp8 of k) -> k8 uint8 [B, H, Lp, 128]: e4m3 bytes of k / scale in
    natural dim order, rows L .. Lp-1 = row L-1 (osk_k_pack_fp8)."""
    assert k.dim() == 3, k.shape
    B, L, C_ = k.shape
    assert hd == 128, f"the fp8 QK^T kernel exists for head_dim 128 only, not {hd}"
    assert k.dtype == torch.bfloat16 and C_ == H * hd, (k.dtype, k.shape)
    assert k.stride(2) == 1 and k.stride(0) % 8 == 0 and k.stride(1) % 8 == 0 and k.data_ptr() % 16 == 0, (k.stride(), k.data_ptr() % 16)
    assert k8.dtype == torch.uint8 and k8.is_contiguous() and tuple(k8.shape) == k8_shape(B, H, L, hd) and k8.data_ptr() % 16 == 0, (k8.dtype, k8.shape)
    assert scales.dtype == torch.float32 and scales.is_contiguous() and scales.numel() == B * H, (scales.dtype, scales.shape)
    _check(lib.osk_k_pack_fp8(k.data_ptr(), k.stride(0), k.stride(1), scales.data_ptr(), k8.data_ptr(), B, L, H, hd, _stream()),
           "osk_k_pack_fp8")
    return k8


def kv_quant_rows_fp8(x: torch.Tensor, scales: torch.Tensor, out: torch.Tensor, H: int, hd: int) -> torch.Tensor:
    """x bf16 [B, L, H*hd] view, scales f32 [B, H] -> out uint8 [B, L, H*hd] view (its own batch / row strides: a slot of a gather
    buffer): the e4m3 bytes of x / scale, token-major, each byte the one k_pack_fp8 / v_transpose_fp8 produce for that element
    (osk_kv_quant_rows_fp8).  head_dim 72 / 128."""
    assert x.dim() == 3 and out.dim() == 3, (x.shape, out.shape)
    B, L, C_ = x.shape
    al = 16 if hd == 128 else 8
    assert x.dtype == torch.bfloat16 and C_ == H * hd and hd in (72, 128), (x.dtype, x.shape, H, hd)
    assert x.stride(2) == 1 and x.stride(0) % 8 == 0 and x.stride(1) % 8 == 0 and x.data_ptr() % 16 == 0, (x.stride(), x.data_ptr() % 16)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B, L, C_) and out.device == x.device, (out.dtype, out.shape)
    assert out.stride(2) == 1 and out.stride(0) % al == 0 and out.stride(1) % al == 0 and out.data_ptr() % al == 0, (out.stride(), out.data_ptr() % al)
    assert scales.dtype == torch.float32 and scales.is_contiguous() and scales.numel() == B * H, (scales.dtype, scales.shape)
    _check(lib.osk_kv_quant_rows_fp8(x.data_ptr(), x.stride(0), x.stride(1), scales.data_ptr(), out.data_ptr(), out.stride(0),
                                     out.stride(1), B, L, H, hd, _stream()), "osk_kv_quant_rows_fp8")
    return out


def kv_join_fp8(k_seg: torch.Tensor, v_seg: torch.Tensor, k_out: torch.Tensor, vt8_out: torch.Tensor, H: int, hd: int, L: int):
    """the gathered segments [n_seg, B, seg_len, H*hd] (key j in segment j // seg_len, row j % seg_len; (n_seg - 1) * seg_len < L <=
    n_seg * seg_len) -> the fp8 operands of one key segment of L keys (osk_kv_join_fp8): v_seg uint8 (kv_quant_rows_fp8 bytes) ->
    vt8_out uint8 [B, H, vt8_rows(hd), round_up(L, 64)], bit for bit v_transpose_fp8 of the L keys as one contiguous V; k_seg uint8
    (head_dim 128) -> k_out = k8 uint8 [B, H, round_up(L, 64), 128], bit for bit k_pack_fp8; k_seg bf16 -> k_out the bf16 [B, L, H*hd]
    view kv_join writes.  The K kind is k_seg's dtype."""
    n_seg, B, seg_len, D = v_seg.shape
    k8 = k_seg.dtype == torch.uint8
    al = 16 if hd == 128 else 8
    assert hd in (72, 128) and D == H * hd and (hd == 128 or not k8), (D, H, hd, k_seg.dtype)
    assert v_seg.dtype == torch.uint8 and v_seg.stride(3) == 1 and all(s % al == 0 for s in v_seg.stride()[:3]) and v_seg.data_ptr() % al == 0, (v_seg.dtype, v_seg.stride())
    assert k_seg.dtype in (torch.uint8, torch.bfloat16) and tuple(k_seg.shape) == (n_seg, B, seg_len, D) and k_seg.stride(3) == 1, (k_seg.dtype, k_seg.shape)
    assert all(s % (16 if k8 else 8) == 0 for s in k_seg.stride()[:3]) and k_seg.data_ptr() % 16 == 0, k_seg.stride()
    Lp = (L + 63) // 64 * 64
    if k8:
        assert k_out.dtype == torch.uint8 and tuple(k_out.shape) == k8_shape(B, H, L, hd) and k_out.is_contiguous(), (k_out.dtype, k_out.shape)
        kobs = kors = 0
    else:
        assert k_out.dtype == torch.bfloat16 and tuple(k_out.shape) == (B, L, D) and k_out.stride(2) == 1, (k_out.dtype, k_out.shape, k_out.stride())
        assert k_out.stride(0) % 8 == 0 and k_out.stride(1) % 8 == 0, k_out.stride()
        kobs, kors = k_out.stride(0), k_out.stride(1)
    assert k_out.data_ptr() % 16 == 0 and vt8_out.data_ptr() % 16 == 0
    assert vt8_out.dtype == torch.uint8 and tuple(vt8_out.shape) == (B, H, vt8_rows(hd), Lp) and vt8_out.is_contiguous(), (vt8_out.dtype, vt8_out.shape)
    assert (n_seg - 1) * seg_len < L <= n_seg * seg_len, (n_seg, seg_len, L)
    _check(lib.osk_kv_join_fp8(k_seg.data_ptr(), k_seg.stride(0), k_seg.stride(1), k_seg.stride(2), int(k8), v_seg.data_ptr(),
                               v_seg.stride(0), v_seg.stride(1), v_seg.stride(2), k_out.data_ptr(), kobs, kors, vt8_out.data_ptr(),
                               B, H, hd, n_seg, seg_len, L, _stream()), "osk_kv_join_fp8")


def attention_fwd_qk8(q: torch.Tensor, k8: torch.Tensor, k_scale: torch.Tensor, vt8: torch.Tensor, v_scale: torch.Tensor,
                      out: torch.Tensor, H: int, hd: int, scale: float, *, seg_len: int, lse=None, n_seg: int = 1,
                      k_seg_stride: int = 0, vt_seg_stride: int = 0, q_prescaled: bool = False, kv_batches: int = 0,
                      workspace: torch.Tensor | None = None):
    """attention_fwd_pv8 with QK^T on the fp8 MFMA as well (head_dim 128): k8 / k_scale from k_pack_fp8 -- k8 is segment 0's
    [Bkv, H, Lp, 128] tensor, further segments k_seg_stride BYTES apart; seg_len = keys per segment (k8 only shows Lp)."""
    # (lse: this wrapper has never looked at its shape)
    kbs, krs = _attn_operands(2, q, k8, k_scale, vt8, v_scale, out, None, H, hd, kv_batches, seg_len, k_seg_stride, vt_seg_stride,
                              vt_keys=(seg_len + 63) // 64 * 64)
    B, Lq, _ = q.shape
    with _attn_prof():
        _check(lib.osk_attention_fwd_qk8_bf16(q.data_ptr(), q.stride(0), q.stride(1), k8.data_ptr(), k_seg_stride, kbs, krs,
                                              k_scale.data_ptr(), vt8.data_ptr(), vt_seg_stride, v_scale.data_ptr(), out.data_ptr(),
                                              out.stride(0), out.stride(1), _p(lse), B, H, Lq, n_seg, seg_len, hd, scale,
                                              int(q_prescaled), kv_batches, _p(workspace),
                                              0 if workspace is None else workspace.numel(), _stream()), "osk_attention_fwd_qk8_bf16")
    return out


ATTN_MODES = {"pv8": 1, "qk8": 2}     # OSK_ATTN_PV8, OSK_ATTN_QK8 of include/osk.h


def attention_fwd_window_fp8(q: torch.Tensor, k: torch.Tensor, k_scale: torch.Tensor | None, vt8: torch.Tensor, v_scale: torch.Tensor,
                             out: torch.Tensor, H: int, hd: int, scale: float, *, n_prefix: int, windows: torch.Tensor, mode: str,
                             lse=None, q_prescaled: bool = False, kv_batches: int = 0, workspace: torch.Tensor | None = None,
                             Lk: int | None = None):
    """attention_fwd_window on fp8 operands (osk_attention_fwd_window_fp8_bf16): the same mask -- query block i sees keys
    [0, n_prefix) and the body tiles windows[i] = (first, count), nothing else -- with the kernels of attention_fwd_pv8 (mode "pv8",
    head_dim 72 / 128: k the bf16 [Bkv, Lk, H*hd] view, k_scale None) or attention_fwd_qk8 (mode "qk8", head_dim 128: k = k8
    [Bkv, H, Lp, 128] from k_pack_fp8 of all Lk keys, k_scale its scales, Lk = the key count -- k8 only shows Lp, as seg_len of
    attention_fwd_qk8).  vt8 / v_scale: v_transpose_fp8 of all Lk keys.  windows, lse, workspace as attention_fwd_window."""
    if mode not in ATTN_MODES:
        raise ValueError(f"attention_fwd_window_fp8: mode {mode!r}, expected 'pv8' or 'qk8'")
    return _attention_window(ATTN_MODES[mode], q, k, k_scale, vt8, v_scale, out, H, hd, scale, n_prefix, windows, lse, q_prescaled,
                             kv_batches, 0.0, workspace, Lk)


def copy_rows_ok(src: torch.Tensor, dst: torch.Tensor) -> bool:
    """every precondition of osk_copy_rows_bf16 (csrc/elementwise.hip): bf16, unit channel stride, C % 4 == 0, all other strides
    % 4 == 0, 8-byte aligned pointers, non-empty -- callers fall back to torch's copy otherwise"""
    if not (src.dtype == dst.dtype == torch.bfloat16 and src.ndim == dst.ndim and src.ndim in (3, 4)):
        return False
    if src.numel() == 0 or src.shape[-1] % 4 or src.stride(-1) != 1 or dst.stride(-1) != 1 or dst.shape[-1] < src.shape[-1]:
        return False
    if any(st % 4 for st in src.stride()[:-1]) or any(st % 4 for st in dst.stride()[:-1]):
        return False
    return src.data_ptr() % 8 == 0 and dst.data_ptr() % 8 == 0


def copy_rows(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst[..., :C] = src for bf16 [B, L, C] -- or [P, B, L, C], P chunks -- views with unit channel stride on both sides (dst rows
    may be wider than C: a column slice of a K-padded operand; either side's chunk axis may be a column group of a token-major
    tensor: `x.view(B, L, P, C).permute(2, 0, 1, 3)`); a 3-D src of batch 1 -- or an expanded view -- is broadcast over dst's batch."""
    assert src.dtype == dst.dtype == torch.bfloat16 and src.ndim == dst.ndim and src.ndim in (3, 4), (src.dtype, dst.dtype, src.shape, dst.shape)
    if src.ndim == 3:
        src, dst = src.unsqueeze(0), dst.unsqueeze(0)
    NC, B, L, Cc = dst.shape[0], dst.shape[1], dst.shape[2], src.shape[3]
    assert src.shape[0] == NC and src.shape[2] == L and src.shape[1] in (1, B) and dst.shape[3] >= Cc and src.stride(3) == 1 and dst.stride(3) == 1
    sbs = 0 if src.shape[1] == 1 else src.stride(1)
    _check(lib.osk_copy_rows_bf16(src.data_ptr(), src.stride(0), sbs, src.stride(2), dst.data_ptr(), dst.stride(0), dst.stride(1), dst.stride(2),
                                  NC, B, L, Cc, _stream()), "osk_copy_rows_bf16")
    return dst


def cfg_euler(pred: torch.Tensor, x: torch.Tensor, x_out: torch.Tensor, g_txt: float, g_img: float, dt: float,
              g_img_vec=None):
    """pred bf16 [3, ...] contiguous (cond, uncond, uncond_2); x, x_out bf16 [...] contiguous."""
    n = x.numel()
    assert pred.numel() == 3 * n and pred.is_contiguous() and x.is_contiguous() and x_out.is_contiguous()
    assert pred.dtype == x.dtype == x_out.dtype == torch.bfloat16, \
        f"osk_cfg_euler_bf16 reads and writes bf16; got {pred.dtype}, {x.dtype}, {x_out.dtype}"
    _check(lib.osk_cfg_euler_bf16(pred.data_ptr(), n, x.data_ptr(), x_out.data_ptr(), g_txt, g_img,
                                  _p(g_img_vec), dt, _stream()), "osk_cfg_euler_bf16")
    return x_out


def cfg_euler_nb(pred: torch.Tensor, nb: int, x: torch.Tensor, x_out: torch.Tensor, g_txt: float, g_img: float, dt: float,
                 g_img_vec=None):
    """pred bf16 contiguous, its first nb chunks of x.numel() elements = the branches that ran (cond[, uncond[, uncond_2]]);
    x, x_out bf16 [...] contiguous.  nb outside 1..3 is refused by the library (RuntimeError), nothing is launched."""
    n = x.numel()
    assert pred.numel() >= max(nb, 1) * n and pred.is_contiguous() and x.is_contiguous() and x_out.is_contiguous()
    assert pred.dtype == x.dtype == x_out.dtype == torch.bfloat16, \
        f"osk_cfg_euler_nb_bf16 reads and writes bf16; got {pred.dtype}, {x.dtype}, {x_out.dtype}"
    assert g_img_vec is None or (g_img_vec.dtype == torch.float32 and g_img_vec.numel() == n and g_img_vec.is_contiguous())
    _check(lib.osk_cfg_euler_nb_bf16(pred.data_ptr(), nb, n, x.data_ptr(), x_out.data_ptr(), g_txt, g_img,
                                     _p(g_img_vec), dt, _stream()), "osk_cfg_euler_nb_bf16")
    return x_out


# ----------------------------------------------------------------------------------------------
# step cache of the sampler (csrc/step_cache.hip)
# ----------------------------------------------------------------------------------------------
def _step_view(t, name: str, what: str) -> None:
    """a bf16 [B, L, C] device view the step-cache kernels take: unit channel stride, C and the other strides multiples of 8, 16-byte
    aligned -- ValueError before anything is launched"""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.bfloat16 and t.ndim == 3 and t.numel() > 0):
        raise ValueError(f"{what}: {name} must be a non-empty bf16 [B, L, C] tensor on the GPU; got "
                         f"{(t.device.type, t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
    if t.shape[2] % 8 or t.stride(2) != 1 or t.stride(0) % 8 or t.stride(1) % 8 or t.data_ptr() % 16:
        raise ValueError(f"{what}: {name} needs C % 8 == 0, unit channel stride, batch / row strides % 8 == 0 and 16-byte alignment; "
                         f"got shape {tuple(t.shape)}, strides {t.stride()}")
    if t.numel() // 8 >= 2 ** 31:
        raise ValueError(f"{what}: {name} has {t.numel()} elements; the kernels index up to 2^34")


def step_delta_workspace_bytes(B: int, L: int, C: int) -> int:
    return int(lib.osk_step_delta_workspace_bytes(B, L, C))


def step_delta(cur: torch.Tensor, prev: torch.Tensor, sums: torch.Tensor, workspace: torch.Tensor) -> torch.Tensor:
    """sums f32 [2] = (sum |cur - prev|, sum |prev|), then prev := cur: osk_step_delta_bf16.  cur a bf16 [B, L, C] view, prev
    contiguous of the same shape, workspace a uint8 tensor of step_delta_workspace_bytes(B, L, C).  Deterministic, capturable."""
    what = "osk_step_delta_bf16"
    _step_view(cur, "cur", what)
    _step_view(prev, "prev", what)
    if prev.shape != cur.shape or not prev.is_contiguous():
        raise ValueError(f"{what}: prev must be contiguous and shaped like cur; got {tuple(prev.shape)} (strides {prev.stride()}) for {tuple(cur.shape)}")
    if not (torch.is_tensor(sums) and sums.is_cuda and sums.dtype == torch.float32 and sums.numel() == 2 and sums.is_contiguous()):
        raise ValueError(f"{what}: sums must be a contiguous f32 [2] tensor on the GPU")
    B, L, Cc = cur.shape
    if not (torch.is_tensor(workspace) and workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()
            and workspace.numel() >= step_delta_workspace_bytes(B, L, Cc) and workspace.data_ptr() % 4 == 0):
        raise ValueError(f"{what}: workspace must be a uint8 tensor on the GPU of at least step_delta_workspace_bytes({B}, {L}, {Cc}) bytes")
    lo, hi = cur.data_ptr(), cur.data_ptr() + 2 * ((B - 1) * cur.stride(0) + (L - 1) * cur.stride(1) + Cc)
    if lo < prev.data_ptr() + 2 * prev.numel() and prev.data_ptr() < hi:
        raise ValueError(f"{what}: cur and prev overlap")
    _check(lib.osk_step_delta_bf16(cur.data_ptr(), cur.stride(0), cur.stride(1), prev.data_ptr(), sums.data_ptr(), B, L, Cc,
                                   workspace.data_ptr(), workspace.numel(), _stream()), what)
    return sums


def step_sums_combine(pairs: torch.Tensor, sums: torch.Tensor) -> torch.Tensor:
    """sums f32 [2] = the P rows of pairs f32 [P, 2] added in row order with plain f32 adds on one lane: osk_step_sums_combine_f32.
    The ranks of a sharded step cache each hold the same gathered pairs, so they get the same bits.  Deterministic, capturable."""
    what = "osk_step_sums_combine_f32"
    if not (torch.is_tensor(pairs) and pairs.is_cuda and pairs.dtype == torch.float32 and pairs.ndim == 2 and pairs.shape[0] >= 1
            and pairs.shape[1] == 2 and pairs.is_contiguous()):
        raise ValueError(f"{what}: pairs must be a contiguous f32 [P, 2] tensor on the GPU with P >= 1")
    if not (torch.is_tensor(sums) and sums.is_cuda and sums.dtype == torch.float32 and sums.numel() == 2 and sums.is_contiguous()):
        raise ValueError(f"{what}: sums must be a contiguous f32 [2] tensor on the GPU")
    if sums.data_ptr() < pairs.data_ptr() + 4 * pairs.numel() and pairs.data_ptr() < sums.data_ptr() + 8:
        raise ValueError(f"{what}: sums and pairs overlap")
    _check(lib.osk_step_sums_combine_f32(pairs.data_ptr(), pairs.shape[0], sums.data_ptr(), _stream()), what)
    return sums


def _residual(fn, what: str, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    for t, name in ((a, "a"), (b, "b"), (out, "out")):
        _step_view(t, name, what)
    if not (a.shape == b.shape == out.shape):
        raise ValueError(f"{what}: a, b and out must have one shape; got {tuple(a.shape)}, {tuple(b.shape)}, {tuple(out.shape)}")
    for t, name in ((a, "a"), (b, "b")):
        if t.data_ptr() == out.data_ptr() and t.stride() != out.stride():
            raise ValueError(f"{what}: out aliases {name} with other strides")
    B, L, Cc = a.shape
    _check(fn(a.data_ptr(), a.stride(0), a.stride(1), b.data_ptr(), b.stride(0), b.stride(1), out.data_ptr(), out.stride(0), out.stride(1),
              B, L, Cc, _stream()), what)
    return out


def residual_sub(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out = bf16(f32(a) - f32(b)) over bf16 [B, L, C] views, one rounding; out may be a or b"""
    return _residual(lib.osk_residual_sub_bf16, "osk_residual_sub_bf16", a, b, out)


def residual_add(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out = bf16(f32(a) + f32(b)) over bf16 [B, L, C] views, one rounding; out may be a or b"""
    return _residual(lib.osk_residual_add_bf16, "osk_residual_add_bf16", a, b, out)


# ----------------------------------------------------------------------------------------------
# attention broadcast of the sampler (csrc/attn_cache.hip)
# ----------------------------------------------------------------------------------------------
def attn_cache_copy(src: torch.Tensor, dst: torch.Tensor, row_map: torch.Tensor | None, to_cache: bool) -> torch.Tensor:
    """osk_attn_cache_copy_bf16 over bf16 [., L, C] views.  to_cache (store): src [B, L, C] is the step's attention output, dst the
    cache slot [cache_rows, L, C], dst[row_map[b]] = src[b].  Otherwise (load): src is the slot, dst [B, L, C], dst[b] =
    src[row_map[b]].  row_map: int32 [B] on the device with distinct entries in [0, cache_rows), or None for the identity.  The
    map is read on the device (a captured graph replays it); its values are the caller's to get right -- an entry outside the
    slot makes the kernel skip that batch item.  Capturable."""
    what = "osk_attn_cache_copy_bf16"
    _step_view(src, "src", what)
    _step_view(dst, "dst", what)
    step, slot = (src, dst) if to_cache else (dst, src)
    B, L, Cc = step.shape
    if slot.shape[1:] != step.shape[1:]:
        raise ValueError(f"{what}: the slot {tuple(slot.shape)} and the step's view {tuple(step.shape)} differ in L or C")
    if row_map is None:
        if B > slot.shape[0]:
            raise ValueError(f"{what}: {B} batch items do not fit a slot of {slot.shape[0]} rows")
    elif not (torch.is_tensor(row_map) and row_map.is_cuda and row_map.dtype == torch.int32 and row_map.ndim == 1 and row_map.numel() == B
              and row_map.is_contiguous()):
        raise ValueError(f"{what}: row_map must be a contiguous int32 [{B}] tensor on the GPU (or None)")
    for t, name in ((src, "src"), (dst, "dst")):
        if t.shape[0] > 1 and t.stride(0) < L * t.stride(1) or t.stride(1) < Cc:
            raise ValueError(f"{what}: {name}'s rows or batch items overlap (strides {t.stride()})")
    ext = lambda t: (t.data_ptr(), t.data_ptr() + 2 * ((t.shape[0] - 1) * t.stride(0) + (L - 1) * t.stride(1) + Cc))
    (s0, s1), (d0, d1) = ext(src), ext(dst)
    if s0 < d1 and d0 < s1:
        raise ValueError(f"{what}: src and dst overlap")
    _check(lib.osk_attn_cache_copy_bf16(src.data_ptr(), src.stride(0), src.stride(1), dst.data_ptr(), dst.stride(0), dst.stride(1),
                                        _p(row_map), slot.shape[0], 1 if to_cache else 0, B, L, Cc, _stream()), what)
    return dst


# ----------------------------------------------------------------------------------------------
# causal 3-D VAE kernels (NDHWC bf16)
# ----------------------------------------------------------------------------------------------
# bench.py sets this to a list to collect (start, end, padded-channel FLOPs) around every conv launch
PROFILE_CONV = None


def conv_out_dims(T: int, H: int, W: int, stride=(1, 1, 1), up=(False, False)):
    Tu = 1 + 2 * (T - 1) if up[0] else T
    Hu, Wu = (2 * H, 2 * W) if up[1] else (H, W)
    return (Tu - 1) // stride[0] + 1, (Hu - 1) // stride[1] + 1, (Wu - 1) // stride[2] + 1


def causal_conv3d(x: torch.Tensor, w: torch.Tensor, bias, out: torch.Tensor, ksize: int, stride=(1, 1, 1),
                  up=(False, False), res=None, gn_sums: torch.Tensor | None = None) -> torch.Tensor:
    """x bf16 [B, T, H, W, Cin] contiguous; w bf16 [Cout, Kpad] (tap-major, channel-minor, zero padded);
    bias f32 [Cout] | None; out bf16 [B, To, Ho, Wo, Cout] contiguous; res like out | None.
    gn_sums (f64 [B, G, 2], zeroed by the caller): also accumulate the GroupNorm statistics of `out` in the conv's
    epilogue; the return value is then (out, fused).  The kernels that carry that epilogue do not take every shape: when
    they do not, the plain conv runs, gn_sums stays untouched and fused is False (the consumer runs groupnorm_stats)."""
    B, T, H, W, Cin = x.shape
    Cout = w.shape[0]
    To, Ho, Wo = conv_out_dims(T, H, W, stride, up)
    assert x.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (B, To, Ho, Wo, Cout), (out.shape, (B, To, Ho, Wo, Cout))
    assert res is None or (res.is_contiguous() and res.shape == out.shape)
    prof = PROFILE_CONV
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    fused = False
    if gn_sums is not None:
        assert gn_sums.dtype == torch.float64 and gn_sums.is_contiguous() and gn_sums.shape[0] == B and gn_sums.shape[2] == 2
        rc = lib.osk_causal_conv3d_gn_ndhwc_bf16(x.data_ptr(), B, T, H, W, Cin, w.data_ptr(), w.stride(0), _p(bias), Cout,
                                                 ksize, stride[0], stride[1], stride[2], int(up[0]), int(up[1]), _p(res),
                                                 out.data_ptr(), To, Ho, Wo, gn_sums.data_ptr(), gn_sums.shape[1], _stream())
        fused = rc == 0
        if rc != 0 and rc != OSK_EUNSUPPORTED:
            _check(rc, "osk_causal_conv3d_gn_ndhwc_bf16")
    if not fused:
        _check(lib.osk_causal_conv3d_ndhwc_bf16(x.data_ptr(), B, T, H, W, Cin, w.data_ptr(), w.stride(0), _p(bias), Cout,
                                                ksize, stride[0], stride[1], stride[2], int(up[0]), int(up[1]), _p(res),
                                                out.data_ptr(), To, Ho, Wo, _stream()), "osk_causal_conv3d_ndhwc_bf16")
    if prof is not None:
        ev1.record()
        prof.append((ev0, ev1, 2.0 * Cin * Cout * ksize ** 3 * B * To * Ho * Wo))
    return out if gn_sums is None else (out, fused)


CONV_KERNEL_CLASSES = ("tile128", "tile128_bigc", "fewout", "conv256x4", "conv256x8", "convsw4", "convsw8", "convsw4_up", "convsw8_up",
                       "convsw8_gn", "convsw2", "convsw2_gn")     # OSK_CONV_* of include/osk.h, by value


def conv_kernel_class(B: int, T: int, H: int, W: int, Cin: int, Cout: int, ksize: int, stride=(1, 1, 1), up=(False, False), *,
                      w_row_stride: int | None = None, out_align: int = 16, res_align: int = 0, gn_groups: int = 0,
                      gn_in: bool = False):
    """Host only: the kernel osk_causal_conv3d*_ndhwc_bf16 launch for this call, from the selection code the launch itself switches
    on -> (name in CONV_KERNEL_CLASSES, fused statistics on), or the negative status the entry point would return (nothing
    launched).  out_align / res_align: byte alignment of out / res (res_align 0 = no residual); gn_groups > 0 = gn_sums given."""
    To, Ho, Wo = conv_out_dims(T, H, W, stride, up)
    if w_row_stride is None:
        w_row_stride = (ksize ** 3 * Cin + 63) // 64 * 64
    rc = lib.osk_causal_conv3d_kernel_class(B, T, H, W, Cin, w_row_stride, Cout, ksize, stride[0], stride[1], stride[2], int(up[0]),
                                            int(up[1]), To, Ho, Wo, out_align, res_align, gn_groups, int(gn_in))
    return rc if rc < 0 else (CONV_KERNEL_CLASSES[rc & 0xFF], bool(rc & 0x100))


def causal_conv3d_gn_in(x: torch.Tensor, table: torch.Tensor, w: torch.Tensor, bias, out: torch.Tensor, ksize: int,
                        stride=(1, 1, 1), res=None, gn_sums: torch.Tensor | None = None):
    """conv(silu(GroupNorm(x))) reading x itself: `table` (groupnorm_table) carries the norm's per-(batch, channel) scale / shift and
    the sliding-window kernels apply it -- with the rounding points of groupnorm_apply(silu=True) -- while they refill their halo.
    -> (ran, fused): ran False = the shape is not one those kernels take and NOTHING was launched (the caller runs
    groupnorm_apply + causal_conv3d); fused = gn_sums was accumulated in the epilogue as in causal_conv3d."""
    B, T, H, W, Cin = x.shape
    Cout = w.shape[0]
    To, Ho, Wo = conv_out_dims(T, H, W, stride)
    assert x.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (B, To, Ho, Wo, Cout), (out.shape, (B, To, Ho, Wo, Cout))
    assert res is None or (res.is_contiguous() and res.shape == out.shape)
    assert table.dtype == torch.float32 and table.is_contiguous() and tuple(table.shape) == (B, Cin // 8, 16), table.shape
    prof = PROFILE_CONV
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()

    def call(sums):
        return lib.osk_causal_conv3d_gnin_ndhwc_bf16(x.data_ptr(), table.data_ptr(), B, T, H, W, Cin, w.data_ptr(), w.stride(0),
                                                     _p(bias), Cout, ksize, stride[0], stride[1], stride[2], _p(res),
                                                     out.data_ptr(), To, Ho, Wo, _p(sums), 0 if sums is None else sums.shape[1],
                                                     _stream())

    fused = False
    rc = OSK_EUNSUPPORTED
    if gn_sums is not None:
        assert gn_sums.dtype == torch.float64 and gn_sums.is_contiguous() and gn_sums.shape[0] == B and gn_sums.shape[2] == 2
        rc = call(gn_sums)
        fused = rc == 0
    if rc == OSK_EUNSUPPORTED:
        rc = call(None)
    if rc == OSK_EUNSUPPORTED:
        return False, False
    _check(rc, "osk_causal_conv3d_gnin_ndhwc_bf16")
    if prof is not None:
        ev1.record()
        prof.append((ev0, ev1, 2.0 * Cin * Cout * ksize ** 3 * B * To * Ho * Wo))
    return True, fused


def conv2d(x: torch.Tensor, w: torch.Tensor, bias, out: torch.Tensor, ksize: int, stride: int = 1, pad: int = 1, up: bool = False,
           res=None) -> torch.Tensor:
    """zero-padded 2-D conv, NHWC bf16.  x [B, H, W, Cin] contiguous, Cin = 8 * 2^j; w bf16 [Cout, Kpad] (tap-major,
    channel-minor, zero padded); bias f32 [Cout] | None; out bf16 [B, Ho, Wo, Cout] contiguous (its extent is the caller's: `pad`
    zero rows / columns in front, zeros behind as far as the extent reads); res like out | None.  The C entry's fused-statistics
    argument is not bound: the kernel has no such epilogue (osk.h)."""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = out.shape[1], out.shape[2]
    assert x.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (B, Ho, Wo, Cout), (out.shape, (B, Ho, Wo, Cout))
    assert res is None or (res.is_contiguous() and res.shape == out.shape)
    prof = PROFILE_CONV
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    _check(lib.osk_conv2d_nhwc_bf16(x.data_ptr(), B, H, W, Cin, w.data_ptr(), w.stride(0), _p(bias), Cout, ksize, stride, pad,
                                    int(up), _p(res), out.data_ptr(), Ho, Wo, None, 0, _stream()), "osk_conv2d_nhwc_bf16")
    if prof is not None:
        ev1.record()
        prof.append((ev0, ev1, 2.0 * Cin * Cout * ksize ** 2 * B * Ho * Wo))
    return out


def groupnorm_table(sums: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, table: torch.Tensor, S: int, G: int,
                    eps: float = 1e-6) -> torch.Tensor:
    """sums f64 [B, G, 2] over S voxels -> table f32 [B, C / 8, 16]: per 8-channel chunk 8 scales rstd gamma, 8 shifts beta - mean
    rstd gamma (the constants groupnorm_apply derives), for causal_conv3d_gn_in."""
    B, C = sums.shape[0], gamma.numel()
    assert table.dtype == torch.float32 and table.is_contiguous() and tuple(table.shape) == (B, C // 8, 16), table.shape
    _check(lib.osk_groupnorm_table_f32(sums.data_ptr(), gamma.data_ptr(), beta.data_ptr(), table.data_ptr(), B, S, C, G, eps,
                                       _stream()), "osk_groupnorm_table_f32")
    return table


def groupnorm_stats(x: torch.Tensor, G: int, sums: torch.Tensor) -> torch.Tensor:
    """x bf16 [B, ..., C] contiguous -> sums f64 [B, G, 2]."""
    B, C = x.shape[0], x.shape[-1]
    S = x.numel() // (B * C)
    _check(lib.osk_groupnorm_stats_ndhwc_bf16(x.data_ptr(), B, S, C, G, sums.data_ptr(), _stream()),
           "osk_groupnorm_stats_ndhwc_bf16")
    return sums


def groupnorm_apply(x: torch.Tensor, sums: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out: torch.Tensor,
                    G: int, eps: float = 1e-6, silu: bool = True) -> torch.Tensor:
    B, C = x.shape[0], x.shape[-1]
    S = x.numel() // (B * C)
    _check(lib.osk_groupnorm_apply_ndhwc_bf16(x.data_ptr(), sums.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                              out.data_ptr(), B, S, C, G, eps, 1 if silu else 0, _stream()),
           "osk_groupnorm_apply_ndhwc_bf16")
    return out


def masked_softmax(scores: torch.Tensor, probs: torch.Tensor, Sk: int, keys_per_frame: int, scale: float):
    """scores f32 [Sq, >=Sk] (row stride arbitrary), probs bf16 [Sq, ldp] contiguous rows, ldp >= Sk."""
    Sq = scores.shape[0]
    _check(lib.osk_masked_softmax_f32_bf16(scores.data_ptr(), scores.stride(0), probs.data_ptr(), probs.stride(0), Sq,
                                           Sk, keys_per_frame, scale, _stream()), "osk_masked_softmax_f32_bf16")
    return probs


def blend(a: torch.Tensor, b: torch.Tensor, extent: int, dim: int) -> torch.Tensor:
    """tile cross-fade along `dim`, written into b: the last `extent` slices of a fade into the first `extent` of b.
    a, b: contiguous bf16 tensors that agree in every other dimension."""
    dim = dim % b.ndim
    extent = min(a.shape[dim], b.shape[dim], extent)
    if extent == 0:
        return b
    assert a.dtype == b.dtype == torch.bfloat16 and a.is_contiguous() and b.is_contiguous()
    assert a.shape[:dim] == b.shape[:dim] and a.shape[dim + 1:] == b.shape[dim + 1:], (a.shape, b.shape, dim)
    outer = 1
    for s_ in b.shape[:dim]:
        outer *= s_
    inner = 1
    for s_ in b.shape[dim + 1:]:
        inner *= s_
    _check(lib.osk_blend_bf16(a.data_ptr(), b.data_ptr(), outer, a.shape[dim], b.shape[dim], extent, inner, _stream()),
           "osk_blend_bf16")
    return b


_HD512_WS: dict = {}


def attention_hd512_workspace(B: int, S: int, device) -> torch.Tensor:
    """workspace of the key-split launch, one per (device, stream, size); reused by every call"""
    dev = torch.device(device)
    key = (str(dev), torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0, B, S)
    ws = _HD512_WS.get(key)
    if ws is None:
        if len(_HD512_WS) >= 4:
            _HD512_WS.pop(next(iter(_HD512_WS)))
        ws = _HD512_WS[key] = torch.empty(int(lib.osk_attention_hd512_workspace_bytes(B, S)), dtype=torch.uint8, device=dev)
    return ws


def attention_hd512(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, bias_v, out: torch.Tensor, keys_per_frame: int,
                    scale: float, workspace: torch.Tensor | None = None) -> torch.Tensor:
    """the VAE mid block's one-head attention: q, k, out bf16 [B, S, 512] views; vt bf16 [B, 512, ld] (natural key order,
    zero beyond S, ld >= round_up(S, 32)); bias_v f32 [512] | None; frame-causal over groups of keys_per_frame keys."""
    B, S, C = q.shape
    assert C == 512 and vt.shape[1] == 512 and vt.stride(2) == 1 and q.stride(2) == 1 and k.stride(2) == 1 and out.stride(2) == 1
    _check(lib.osk_attention_hd512_fwd_ws_bf16(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1),
                                               vt.data_ptr(), vt.stride(0), vt.stride(1), _p(bias_v), out.data_ptr(),
                                               out.stride(0), out.stride(1), B, S, keys_per_frame, scale, _p(workspace),
                                               0 if workspace is None else workspace.numel() * workspace.element_size(), _stream()),
           "osk_attention_hd512_fwd_ws_bf16")
    return out


# ----------------------------------------------------------------------------------------------
# Video DC-AE decoder and encoder (csrc/dc_ae.hip)
# ----------------------------------------------------------------------------------------------
def conv3d_zp(x: torch.Tensor, w: torch.Tensor, bias, out: torch.Tensor, ksize: int, up_t: bool = False, up_hw: bool = False,
              silu: bool = False, res=None) -> torch.Tensor:
    """zero-padded stride-1 "same" 3-D conv, NDHWC bf16.  x [B, T, H, W, Cin] contiguous, Cin = 8 * 2^j; w bf16 [Cout, Kpad]
    (tap-major, channel-minor, zero padded); bias f32 [Cout] | None; out bf16 [B, T << up_t, H << up_hw, W << up_hw, Cout];
    res like out | None (added after the optional SiLU)."""
    B, T, H, W, Cin = x.shape
    Cout = w.shape[0]
    want = (B, T << int(up_t), H << int(up_hw), W << int(up_hw), Cout)
    assert x.is_contiguous() and out.is_contiguous() and tuple(out.shape) == want, (out.shape, want)
    assert x.dtype == w.dtype == out.dtype == torch.bfloat16
    assert res is None or (res.is_contiguous() and res.shape == out.shape and res.dtype == torch.bfloat16)
    prof = PROFILE_CONV
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    _check(lib.osk_conv3d_zp_ndhwc_bf16(x.data_ptr(), B, T, H, W, Cin, w.data_ptr(), w.stride(0), _p(bias), Cout, ksize, int(up_t),
                                        int(up_hw), int(silu), _p(res), out.data_ptr(), _stream()), "osk_conv3d_zp_ndhwc_bf16")
    if prof is not None:
        ev1.record()
        prof.append((ev0, ev1, 2.0 * Cin * Cout * ksize ** 3 * out.numel() / Cout))
    return out


def conv3d_zp_strided(x: torch.Tensor, w: torch.Tensor, bias, out: torch.Tensor, stride_t: int, res=None) -> torch.Tensor:
    """zero-padded k = 3 conv with stride (stride_t, 2, 2), NDHWC bf16.  x [B, T, H, W, Cin] contiguous, Cin = 8 * 2^j; w, bias as
    for conv3d_zp; out bf16 [B, (T-1)//stride_t + 1, (H-1)//2 + 1, (W-1)//2 + 1, Cout]; res like out | None."""
    B, T, H, W, Cin = x.shape
    Cout = w.shape[0]
    want = (B, (T - 1) // stride_t + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cout)
    assert x.is_contiguous() and out.is_contiguous() and tuple(out.shape) == want, (out.shape, want)
    assert x.dtype == w.dtype == out.dtype == torch.bfloat16
    assert res is None or (res.is_contiguous() and res.shape == out.shape and res.dtype == torch.bfloat16)
    prof = PROFILE_CONV
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    _check(lib.osk_conv3d_zp_strided_ndhwc_bf16(x.data_ptr(), B, T, H, W, Cin, w.data_ptr(), w.stride(0), _p(bias), Cout,
                                                int(stride_t), 2, _p(res), out.data_ptr(), _stream()),
           "osk_conv3d_zp_strided_ndhwc_bf16")
    if prof is not None:
        ev1.record()
        prof.append((ev0, ev1, 2.0 * Cin * Cout * 27 * out.numel() / Cout))
    return out


def unshuffle_avg(x: torch.Tensor, out: torch.Tensor, ft: int, fhw: int) -> torch.Tensor:
    """pixel-unshuffle channel averaging: x bf16 [B, T, H, W, Cin] -> out bf16 [B, T/ft, H/fhw, W/fhw, Cout]"""
    B, T, H, W, Cin = x.shape
    Cout = out.shape[-1]
    assert T % ft == 0 and H % fhw == 0 and W % fhw == 0, (x.shape, ft, fhw)
    assert x.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (B, T // ft, H // fhw, W // fhw, Cout), out.shape
    assert x.dtype == out.dtype == torch.bfloat16
    _check(lib.osk_unshuffle_avg_ndhwc_bf16(x.data_ptr(), B, T, H, W, Cin, out.data_ptr(), Cout, ft, fhw, _stream()),
           "osk_unshuffle_avg_ndhwc_bf16")
    return out


def dup_shuffle(x: torch.Tensor, out: torch.Tensor, ft: int, fhw: int) -> torch.Tensor:
    """channel-duplicating pixel shuffle: x bf16 [B, T, H, W, Cin] -> out bf16 [B, T*ft, H*fhw, W*fhw, Cout]"""
    B, T, H, W, Cin = x.shape
    Cout = out.shape[-1]
    assert x.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (B, T * ft, H * fhw, W * fhw, Cout), out.shape
    assert x.dtype == out.dtype == torch.bfloat16
    _check(lib.osk_dup_shuffle_ndhwc_bf16(x.data_ptr(), B, T, H, W, Cin, out.data_ptr(), Cout, ft, fhw, _stream()),
           "osk_dup_shuffle_ndhwc_bf16")
    return out


def dwconv3d(x: torch.Tensor, w: torch.Tensor, bias, out: torch.Tensor, ksize: int, glu: bool = False) -> torch.Tensor:
    """depthwise zero-padded conv: x bf16 [B, T, H, W, C]; w bf16 [k^3, C]; bias f32 [C] | None; out bf16 [B, T, H, W, C or C / 2]"""
    B, T, H, W, C = x.shape
    assert x.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (B, T, H, W, C // 2 if glu else C), out.shape
    assert tuple(w.shape) == (ksize ** 3, C) and w.is_contiguous() and x.dtype == w.dtype == out.dtype == torch.bfloat16
    _check(lib.osk_dwconv3d_ndhwc_bf16(x.data_ptr(), B, T, H, W, C, w.data_ptr(), _p(bias), ksize, int(glu), out.data_ptr(),
                                       _stream()), "osk_dwconv3d_ndhwc_bf16")
    return out


def gconv32(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """block-diagonal 1x1x1 conv (32 -> 32 per group): x, out bf16 [..., C] contiguous; w bf16 [C, 32]"""
    C = x.shape[-1]
    assert x.is_contiguous() and out.is_contiguous() and out.shape == x.shape and tuple(w.shape) == (C, 32) and w.is_contiguous()
    assert x.dtype == w.dtype == out.dtype == torch.bfloat16
    _check(lib.osk_gconv32_bf16(x.data_ptr(), x.numel() // C, C, w.data_ptr(), out.data_ptr(), _stream()), "osk_gconv32_bf16")
    return out


def relu_linear_attn_nsplit(N: int) -> int:
    """runs of tokens the K^T V pass is cut into: one per 512 tokens, at most 64"""
    return max(1, min(64, (N + 511) // 512))


def relu_linear_attn(qkv: torch.Tensor, out: torch.Tensor, eps: float = 1e-15, workspace: torch.Tensor | None = None) -> torch.Tensor:
    """qkv bf16 [B, N, G * 96] contiguous ([q | k | v] groups of 3 x 32); out bf16 [B, N, >= G * 32] view with contiguous last dim
    and rows (the first G * 32 columns are written)."""
    B, N, C3 = qkv.shape
    G = C3 // 96
    assert C3 == G * 96 and qkv.is_contiguous() and qkv.dtype == out.dtype == torch.bfloat16
    assert out.shape[0] == B and out.shape[1] == N and out.stride(2) == 1 and out.stride(0) == N * out.stride(1), out.stride()
    nsplit = relu_linear_attn_nsplit(N)
    need = B * G * nsplit * 1056
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.float32, device=qkv.device)
    _check(lib.osk_relu_linear_attn_bf16(qkv.data_ptr(), B, N, G, out.data_ptr(), out.stride(1), workspace.data_ptr(),
                                         workspace.numel() * 4, nsplit, eps, _stream()), "osk_relu_linear_attn_bf16")
    return out


def rmsnorm_affine(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, eps: float = 1e-5, res=None,
                   relu: bool = False) -> torch.Tensor:
    """x, out, res bf16 [..., C] contiguous; weight, bias f32 [C].  out = act(rmsnorm(x) * weight + bias) + res"""
    C = x.shape[-1]
    assert x.is_contiguous() and out.is_contiguous() and out.shape == x.shape and x.dtype == out.dtype == torch.bfloat16
    assert weight.dtype == bias.dtype == torch.float32 and weight.numel() == bias.numel() == C
    assert res is None or (res.is_contiguous() and res.shape == x.shape and res.dtype == torch.bfloat16)
    _check(lib.osk_rmsnorm_affine_bf16(x.data_ptr(), x.numel() // C, C, weight.data_ptr(), bias.data_ptr(), eps, _p(res), int(relu),
                                       out.data_ptr(), _stream()), "osk_rmsnorm_affine_bf16")
    return out


# ----------------------------------------------------------------------------------------------
# CLIP text encoder kernels
# ----------------------------------------------------------------------------------------------
def _rows_of(t: torch.Tensor):
    """(rows, row stride) of a [..., C] view whose leading axes collapse into equally spaced rows"""
    assert t.dim() >= 2 and t.stride(-1) == 1, (t.shape, t.stride())
    rs = t.stride(-2)
    for d in range(t.dim() - 2):
        assert t.shape[d] == 1 or t.stride(d) == t.stride(d + 1) * t.shape[d + 1], f"rows are not equally spaced: {t.shape} {t.stride()}"
    return t.numel() // t.shape[-1], rs


def layernorm_affine(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """out = bf16((x - mean) * rsqrt(var + eps) * weight + bias) over the last axis (osk_layernorm_affine_bf16); x, out bf16 [..., C]
    views with contiguous last dim and equally spaced rows (a row stride >= C on either side); weight, bias f32 [C]."""
    C = x.shape[-1]
    assert out.shape == x.shape and x.dtype == out.dtype == torch.bfloat16, (x.shape, out.shape, x.dtype, out.dtype)
    assert weight.dtype == bias.dtype == torch.float32 and weight.numel() == bias.numel() == C and weight.is_contiguous() and bias.is_contiguous()
    (M, xrs), (_, ors) = _rows_of(x), _rows_of(out)
    _check(lib.osk_layernorm_affine_bf16(x.data_ptr(), xrs, out.data_ptr(), ors, weight.data_ptr(), bias.data_ptr(), M, C, eps, _stream()),
           "osk_layernorm_affine_bf16")
    return out


def attention_causal(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, H: int, hd: int, scale: float) -> torch.Tensor:
    """softmax over j <= i of scale q k^T, times v: the CLIP text self-attention (osk_attention_causal_bf16); q, k, v, out bf16
    [B, L, H*hd] views with contiguous last dim (q, k, v may be column groups of one fused projection output)."""
    B, L, C = q.shape
    assert C == H * hd and k.shape == q.shape and v.shape == q.shape and out.shape == q.shape, (q.shape, k.shape, v.shape, out.shape)
    assert q.dtype == k.dtype == v.dtype == out.dtype == torch.bfloat16, (q.dtype, k.dtype, v.dtype, out.dtype)
    for t in (q, k, v):
        assert t.stride(2) == 1 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and t.data_ptr() % 16 == 0, (t.stride(), t.data_ptr() % 16)
    assert out.stride(2) == 1 and out.stride(0) % 4 == 0 and out.stride(1) % 4 == 0 and out.data_ptr() % 8 == 0, out.stride()
    _check(lib.osk_attention_causal_bf16(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1), v.data_ptr(),
                                         v.stride(0), v.stride(1), out.data_ptr(), out.stride(0), out.stride(1), B, H, L, hd, scale,
                                         _stream()), "osk_attention_causal_bf16")
    return out


def gemm_quickgelu(a: torch.Tensor, w: torch.Tensor, bias, out: torch.Tensor) -> torch.Tensor:
    """out = bf16(quick_gelu(a w^T + bias)), quick_gelu(v) = v * sigmoid(1.702 v) (osk_gemm_quickgelu_bf16); a bf16 [B, L, K] view,
    w bf16 [N, K], bias f32 [N] | None, out bf16 [B, L, N] view -- gemm()'s operands without an epilogue choice."""
    B, L, K = a.shape
    N = w.shape[0]
    assert out.shape[0] == B and out.shape[1] == L and out.shape[2] == N and w.shape[1] == K
    assert a.dtype == w.dtype == out.dtype == torch.bfloat16, (a.dtype, w.dtype, out.dtype)
    with _gemm_prof(2.0 * B * L * N * K):
        _check(lib.osk_gemm_quickgelu_bf16(a.data_ptr(), a.stride(0), a.stride(1), L, w.data_ptr(), w.stride(0), _p(bias), out.data_ptr(),
                                           out.stride(0), out.stride(1), L, B * L, N, K, _stream()), "osk_gemm_quickgelu_bf16")
    return out


class OskLoraAdapter(C.Structure):
    """include/osk.h::OskLoraAdapter"""
    _fields_ = [("a", _vp), ("a_row_stride", _i64), ("b", _vp), ("b_row_stride", _i64), ("r", _i32), ("scale", _f32)]


def lora_merge(w: torch.Tensor, out: torch.Tensor, adapters) -> torch.Tensor:
    """out = bf16(w + sum_i scale_i B_i A_i) with f32 sums and one rounding (osk_lora_merge_bf16).  w, out bf16 [N, K] views with
    contiguous last dim (row slices of a concatenated weight included; out may be w); adapters: up to 8 tuples (A bf16 [r, K],
    B bf16 [N, r], scale), 1 <= r <= 256.  No adapters: a strided copy."""
    N, K = w.shape
    assert tuple(out.shape) == (N, K) and w.dtype == out.dtype == torch.bfloat16, (w.shape, out.shape, w.dtype, out.dtype)
    assert w.stride(1) == 1 and out.stride(1) == 1, (w.stride(), out.stride())
    adapters = list(adapters)
    arr = (OskLoraAdapter * max(len(adapters), 1))()
    for t, (a, b, scale) in zip(arr, adapters):
        r = a.shape[0]
        assert tuple(a.shape) == (r, K) and tuple(b.shape) == (N, r), (a.shape, b.shape, (N, K))
        assert a.dtype == b.dtype == torch.bfloat16 and a.stride(1) == 1 and b.stride(1) == 1 and a.device == b.device == w.device
        t.a, t.a_row_stride, t.b, t.b_row_stride, t.r, t.scale = a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), r, float(scale)
    _check(lib.osk_lora_merge_bf16(w.data_ptr(), w.stride(0), out.data_ptr(), out.stride(0), N, K, C.addressof(arr), len(adapters),
                                   _stream()), "osk_lora_merge_bf16")
    return out
