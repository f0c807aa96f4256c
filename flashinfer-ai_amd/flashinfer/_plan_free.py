"""What the three plan-free calls share (``trtllm_batch_decode_with_kv_cache[_mla]`` of decode.py,
``trtllm_batch_context_with_kv_cache`` of prefill.py): the workspace carved for a device planner, the argument checks.
``_lib.lib`` and ``_lib.require_gpu_tensor`` are looked up on the module at call time: the CPU tests replace both."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from .utils import _unpack_paged_kv_cache, check_shape_dtype_device


def _device_plan_regions(workspace_buffer: torch.Tensor, plan, workspace_fn: str, name: str) -> None:
    """Carve the int region (work list and CSR page table) and the float region (f32 partial states) a device plan
    needs out of one workspace buffer, and write both into ``plan`` (the params of fi_batch_decode_plan_device, of
    fi_batch_prefill_plan_device or of fi_batch_mla_plan_device; ``workspace_fn`` is the C entry that sizes them,
    ``name`` the call the errors are raised for).  ValueError, with the bytes needed, when the buffer is too small."""
    int_bytes, float_bytes = C.c_size_t(), C.c_size_t()
    _lib.check(getattr(_lib.lib(), workspace_fn)(C.byref(plan), C.byref(int_bytes), C.byref(float_bytes)), name)
    base, have = workspace_buffer.data_ptr(), _lib.nbytes(workspace_buffer)
    int_begin = -base % 16  # both regions 16-byte aligned, whatever the buffer's own alignment
    float_begin = int_begin + (int_bytes.value + 15) // 16 * 16
    need = float_begin + float_bytes.value
    if need > have:
        raise ValueError(f"workspace_buffer is too small: {have} bytes given, {need} bytes needed "
                         f"({int_bytes.value} for the work list and page table, {float_bytes.value} for partial states)")
    plan.int_ws, plan.int_ws_bytes = base + int_begin, int_bytes.value
    plan.float_ws, plan.float_ws_bytes = base + float_begin, have - float_begin


def _refuse_fp4_out_and_shared_kv(name: str, kv_cache, out, out_dtype, o_sf_scale, o_sf_vec_size) -> None:
    """NotImplementedError, by name, for the reference's FP4 output forms and its cache with K and V shared."""
    if out_dtype == "nvfp4" or o_sf_scale is not None or o_sf_vec_size is not None:
        raise NotImplementedError(f"{name}: out_dtype='nvfp4' (o_sf_scale, o_sf_vec_size) is not supported")
    if out is not None and not torch.is_tensor(out):
        raise NotImplementedError(f"{name}: out of type {type(out).__name__} (FP4Tensor) is not supported")
    if torch.is_tensor(kv_cache) and kv_cache.dim() == 5 and kv_cache.shape[1] == 1:
        raise NotImplementedError(f"{name}: the [num_pages, 1, ...] kv_cache with K and V shared is not supported")


def _hnd_cache_views(kv_cache) -> Tuple[torch.Tensor, torch.Tensor]:
    """(k_cache, v_cache) of ``[num_pages, 2, num_kv_heads, page_size, head_dim]`` or of a ``(k, v)`` tuple, on a GPU."""
    if torch.is_tensor(kv_cache):
        if kv_cache.dim() != 5 or kv_cache.shape[1] != 2:
            raise ValueError("kv_cache must be [num_pages, 2, num_kv_heads, page_size, head_dim] or a (k, v) tuple")
    elif not (isinstance(kv_cache, tuple) and len(kv_cache) == 2 and all(t.dim() == 4 for t in kv_cache)):
        raise ValueError("a kv_cache tuple holds k and v, each [num_pages, num_kv_heads, page_size, head_dim]")
    k_cache, v_cache = _unpack_paged_kv_cache(kv_cache, "HND")
    _lib.require_gpu_tensor(k_cache, "kv_cache")
    _lib.require_gpu_tensor(v_cache, "kv_cache")
    return k_cache, v_cache


def _check_block_tables_and_lens(block_tables, seq_lens, workspace_buffer, batch_size: int) -> torch.Tensor:
    """The dense block table, the device-resident lengths (returned as int32) and the workspace of a plan-free call."""
    if block_tables.dtype != torch.int32 or block_tables.dim() != 2 or block_tables.shape[0] != batch_size \
            or block_tables.shape[1] == 0 or block_tables.stride(1) != 1:
        raise ValueError(f"block_tables must be int32 [{batch_size}, max_blocks] with contiguous rows")
    if seq_lens.dtype == torch.uint32:
        seq_lens = seq_lens.view(torch.int32)
    if seq_lens.dtype != torch.int32 or seq_lens.shape != (batch_size,) or not seq_lens.is_contiguous():
        raise ValueError(f"seq_lens must be a contiguous int32 / uint32 tensor of shape [{batch_size}]")
    if not workspace_buffer.is_contiguous():
        raise ValueError("workspace_buffer must be contiguous")
    return seq_lens


def _check_len_fits_block_tables(what: str, max_len: int, max_blocks: int, page_size: int) -> None:
    """ValueError when the caller's ``max_seq_len`` / ``max_kv_len`` (``what``) is more than a block-table row holds."""
    if max_len > max_blocks * page_size:
        raise ValueError(f"{what} {max_len} exceeds what block_tables can hold: {max_blocks} blocks of "
                         f"{page_size} tokens")


def _out_or_empty(out: Optional[torch.Tensor], shape, dtype, device) -> torch.Tensor:
    """``out`` when given, checked for shape, dtype, device and contiguity; a new tensor of that kind otherwise."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    check_shape_dtype_device(out, shape, dtype, device, "out")
    if not out.is_contiguous():
        raise ValueError("out must be contiguous")
    return out


def _one_sinks_tensor(sinks, num_qo_heads: int, device) -> Optional[torch.Tensor]:
    """``sinks`` as one float32 ``[num_qo_heads]`` tensor: given so, or as a one-element list."""
    if isinstance(sinks, (list, tuple)):
        if len(sinks) != 1:
            raise ValueError("sinks is one float32 [num_qo_heads] tensor, or a list holding that one tensor")
        sinks = sinks[0]
    if sinks is not None and (not torch.is_tensor(sinks) or sinks.dtype != torch.float32
                              or sinks.shape != (num_qo_heads,) or not sinks.is_contiguous()
                              or sinks.device != device):
        raise ValueError(f"sinks must be a contiguous float32 tensor of shape [{num_qo_heads}] on {device}")
    return sinks
