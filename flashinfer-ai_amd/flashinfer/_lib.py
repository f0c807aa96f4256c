"""ctypes binding of libfi_mi355.so (the C ABI declared in include/fi_mi355.h).

The reference loads one JIT-built module per kernel specialisation through tvm_ffi
(ref: flashinfer/jit/core.py:247-263); here ONE ahead-of-time library serves every op.  There is no
fallback: if the library is missing every op raises (a CPU path would void the parity claims).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("FI_MI355_LIB", os.path.join(_HERE, "libfi_mi355.so"))
_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "fi_mi355.h"))

# The binding is read from the header, once, here.  This module then holds every struct under its C typedef name
# (fi_paged_kv_t, ...) and every FI_ #define and enumerator under its own name (FI_DP_SPLIT_KV, FI_NEG_INF, ...);
# lib() binds the prototypes.
try:
    with open(_HEADER_PATH) as _f:
        _ABI = _abi.parse(_f.read())
except OSError as e:
    raise ImportError(f"cannot read {_HEADER_PATH}: the binding of libfi_mi355.so is derived from this header") from e
globals().update(_ABI.structs)
globals().update(_ABI.constants)

_TORCH2FI = {
    torch.float16: FI_DTYPE_F16,
    torch.bfloat16: FI_DTYPE_BF16,
    torch.float8_e4m3fn: FI_DTYPE_FP8_E4M3,
    torch.float8_e5m2: FI_DTYPE_FP8_E5M2,
    torch.float32: FI_DTYPE_F32,
}


def fi_dtype(dtype: torch.dtype) -> int:
    try:
        return _TORCH2FI[dtype]
    except KeyError:
        raise ValueError(f"unsupported dtype {dtype} for the MI355X kernels") from None


_lib: Optional[C.CDLL] = None

# every symbol include/fi_mi355.h declares; tests check the library exports all of them
EXPORTED_SYMBOLS = list(_ABI.prototypes)


def _symbols_taking(params_t: type):
    return tuple(n for n, (_, argtypes) in _ABI.prototypes.items() if argtypes[:1] == [C.POINTER(params_t)])


SAMPLING_SYMBOLS = _symbols_taking(fi_sampling_params_t)
ROW_TRANSFORM_SYMBOLS = _symbols_taking(fi_row_transform_params_t)


def lib() -> C.CDLL:
    """Load the library (once).  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"{_LIB_PATH} not found: build it with `make -C flashinfer-ai_amd/csrc -j8` "
            "(or python -c 'import __graft_entry__ as g; g.build()').  There is no CPU fallback."
        )
    l = C.CDLL(_LIB_PATH)
    for name, (restype, argtypes) in _ABI.prototypes.items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = l
    return l


def check(status: int, what: str) -> None:
    """Turn a non-zero status into a Python exception carrying fi_last_error().
    (ref: TVM_FFI_ICHECK / FLASHINFER_ERROR surface as Python exceptions.)"""
    if status != 0:
        msg = lib().fi_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed: {msg}")


def set_option(name: str, value: Optional[int]) -> None:
    """fi_set_option: give a kernel-choice switch of this process (``FI_DECODE_MFMA16``, ``FI_GEMM_*``,
    ``FI_NUM_CUS``) a value; None returns it to what the environment gave it when the library loaded."""
    check(lib().fi_set_option(name.encode(), None if value is None else str(value).encode()), f"set_option({name})")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def nbytes(t: torch.Tensor) -> int:
    """Size of a tensor's elements in bytes: what the C ABI takes wherever it takes a buffer size."""
    return t.numel() * t.element_size()


def current_stream(device: torch.device) -> int:
    """hipStream_t of torch's current stream on `device` (ref: csrc/tvm_ffi_utils.h:256-264)."""
    return torch.cuda.current_stream(device).cuda_stream


def batch_decode_plan(float_ws, int_ws, pinned_int_ws, indptr_host, batch_size, num_qo_heads, num_kv_heads, page_size,
                      enable_cuda_graph, head_dim, q_dtype, kv_dtype, max_grid_hint, window_left, what: str):
    """fi_batch_decode_plan on the float workspace's device; returns the plan_info array.  ``indptr_host`` is the
    host copy of the page-table prefix sums, ``q_dtype`` / ``kv_dtype`` are torch dtypes."""
    info = (C.c_int64 * FI_DECODE_PLAN_INFO_LEN)()
    with torch.cuda.device(float_ws.device):
        check(
            lib().fi_batch_decode_plan(
                float_ws.data_ptr(), nbytes(float_ws), int_ws.data_ptr(), pinned_int_ws.data_ptr(), nbytes(int_ws),
                indptr_host.data_ptr(), batch_size, num_qo_heads, num_kv_heads, page_size, int(enable_cuda_graph),
                head_dim, fi_dtype(q_dtype), fi_dtype(kv_dtype), max_grid_hint, window_left, info,
                current_stream(float_ws.device),
            ),
            what,
        )
    return info


def batch_prefill_plan(float_ws, int_ws, pinned_int_ws, qo_indptr_host, kv_indptr_host, kv_len_arr_host,
                       total_num_rows, batch_size, num_qo_heads, num_kv_heads, page_size, enable_cuda_graph,
                       head_dim_qk, head_dim_vo, causal, window_left, fixed_split_size, disable_split_kv, what: str):
    """fi_batch_prefill_plan on the float workspace's device; returns the plan_info array.  The three index tensors
    are host int32 tensors; ``fixed_split_size`` is -1 for the planner's own choice."""
    info = (C.c_int64 * FI_PREFILL_PLAN_INFO_LEN)()
    with torch.cuda.device(float_ws.device):
        check(
            lib().fi_batch_prefill_plan(
                float_ws.data_ptr(), nbytes(float_ws), int_ws.data_ptr(), pinned_int_ws.data_ptr(), nbytes(int_ws),
                qo_indptr_host.data_ptr(), kv_indptr_host.data_ptr(), kv_len_arr_host.data_ptr(), total_num_rows,
                batch_size, num_qo_heads, num_kv_heads, page_size, int(enable_cuda_graph), head_dim_qk, head_dim_vo,
                int(causal), window_left, fixed_split_size, int(disable_split_kv), info,
                current_stream(float_ws.device),
            ),
            what,
        )
    return info


def require_gpu_tensor(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} must live on a GPU (got {t.device}); the MI355X kernels have no CPU fallback"
        )
