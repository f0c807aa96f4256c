"""Page-table utilities (ref: flashinfer/page.py): sequence lengths, ragged -> COO expansion, and the
K/V append scatter that builds the caches the attention path reads."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple, Union

import torch

from . import _lib
from .utils import _check_kv_layout, _unpack_paged_kv_cache, paged_kv


def get_seq_lens(
    kv_indptr: torch.Tensor, kv_last_page_len: torch.Tensor, page_size: int
) -> torch.Tensor:
    r"""KV length of every request of a paged cache (ref: flashinfer/page.py:224-247).

    ``kv_len = max(num_pages - 1, 0) * page_size + last_page_len``

    Parameters
    ----------
    kv_indptr : torch.Tensor
        The indptr of the paged kv-cache, shape: ``[batch_size + 1]``.
    kv_last_page_len : torch.Tensor
        Entries in the last page of each request, shape: ``[batch_size]``.
    page_size : int
        The size of a page in the paged kv-cache.
    """
    return (
        torch.clamp(kv_indptr[1:] - kv_indptr[:-1] - 1, min=0) * page_size + kv_last_page_len
    )


def get_batch_indices_positions(
    append_indptr: torch.Tensor, seq_lens: torch.Tensor, nnz: int
) -> Tuple[torch.Tensor, torch.Tensor]:
    r"""Convert append indptr and sequence lengths to per-token batch indices and positions.

    >>> append_indptr = torch.tensor([0, 1, 3, 6, 10], dtype=torch.int32, device="cuda:0")
    >>> seq_lens = torch.tensor([5, 5, 5, 5])
    >>> batch_indices, positions = flashinfer.get_batch_indices_positions(append_indptr, seq_lens, 10)
    >>> batch_indices
    tensor([0, 1, 1, 2, 2, 2, 3, 3, 3, 3], device='cuda:0', dtype=torch.int32)
    >>> positions
    tensor([4, 3, 4, 2, 3, 4, 1, 2, 3, 4], device='cuda:0', dtype=torch.int32)

    (ref: flashinfer/page.py:169-221)
    """
    _lib.require_gpu_tensor(append_indptr, "append_indptr")
    batch_size = append_indptr.size(0) - 1
    append_indptr = append_indptr.to(torch.int32).contiguous()
    seq_lens = seq_lens.to(device=append_indptr.device, dtype=torch.int32).contiguous()
    batch_indices = torch.empty((nnz,), device=append_indptr.device, dtype=torch.int32)
    positions = torch.empty((nnz,), device=append_indptr.device, dtype=torch.int32)
    with torch.cuda.device(append_indptr.device):
        _lib.check(
            _lib.lib().fi_get_batch_indices_positions(
                append_indptr.data_ptr(), seq_lens.data_ptr(), batch_size, nnz, batch_indices.data_ptr(),
                positions.data_ptr(), _lib.current_stream(append_indptr.device),
            ),
            "get_batch_indices_positions",
        )
    return batch_indices, positions


def block_sparse_indices_to_vector_sparse_offsets(
    block_sparse_indices: torch.Tensor,
    block_sparse_indptr: torch.Tensor,
    vector_sparse_offsets: torch.Tensor,
    vector_sparse_indptr: torch.Tensor,
    kv_lens: torch.Tensor,
    stride_block: int,
    stride_n: int,
    block_size: int,
) -> torch.Tensor:
    r"""Expand the block indices of a block-sparse KV selection into one offset per token, written to
    ``vector_sparse_offsets`` (which is returned): for request ``b`` and ``pos < kv_lens[b]``

    ``vector_sparse_offsets[vector_sparse_indptr[b] + pos] =
    block_sparse_indices[block_sparse_indptr[b] + pos // block_size] * stride_block + (pos % block_size) * stride_n``

    All five tensors are int32 on one device; ``block_sparse_indptr`` has ``batch_size + 1`` entries.  With
    ``block_size == 1`` nothing is launched: the indices (times ``stride_block``) are the offsets.
    (ref: flashinfer/page.py:49-82, include/flashinfer/page.cuh:287-302)
    """
    if block_size == 1:
        return block_sparse_indices if stride_block == 1 else block_sparse_indices * stride_block
    tensors = (("block_sparse_indices", block_sparse_indices), ("block_sparse_indptr", block_sparse_indptr),
               ("vector_sparse_offsets", vector_sparse_offsets), ("vector_sparse_indptr", vector_sparse_indptr),
               ("kv_lens", kv_lens))
    dev = block_sparse_indices.device
    for name, t in tensors:
        _lib.require_gpu_tensor(t, name)
        if t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous int32 tensor on {dev}")
    batch_size = block_sparse_indptr.size(0) - 1
    if vector_sparse_indptr.numel() < batch_size or kv_lens.numel() < batch_size:
        raise ValueError("vector_sparse_indptr and kv_lens must hold an entry for every request")
    with torch.cuda.device(dev):
        _lib.check(
            _lib.lib().fi_block_sparse_indices_to_vector_sparse_offsets(
                block_sparse_indices.data_ptr(), block_sparse_indptr.data_ptr(), vector_sparse_offsets.data_ptr(),
                vector_sparse_indptr.data_ptr(), kv_lens.data_ptr(), stride_block, stride_n, batch_size, block_size,
                block_sparse_indices.numel(), vector_sparse_offsets.numel(), _lib.current_stream(dev),
            ),
            "block_sparse_indices_to_vector_sparse_offsets",
        )
    return vector_sparse_offsets


def append_paged_kv_cache(
    append_key: torch.Tensor,
    append_value: torch.Tensor,
    batch_indices: torch.Tensor,
    positions: torch.Tensor,
    paged_kv_cache: Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]],
    kv_indices: torch.Tensor,
    kv_indptr: torch.Tensor,
    kv_last_page_len: torch.Tensor,
    kv_layout: str = "NHD",
) -> None:
    r"""Append a batch of key/value rows to a paged KV cache (in place).

    append_key / append_value : ``[nnz, num_kv_heads, head_dim]``
    batch_indices / positions : ``[nnz]`` int32 (see :func:`get_batch_indices_positions`)
    paged_kv_cache : 5-D tensor or ``(k_cache, v_cache)`` tuple, layout per ``kv_layout``
    kv_indices / kv_indptr / kv_last_page_len : the page table AFTER the append (pages must be allocated).
    (ref: flashinfer/page.py:299-425)
    """
    _check_kv_layout(kv_layout)
    for t, name in ((append_key, "append_key"), (append_value, "append_value")):
        _lib.require_gpu_tensor(t, name)
    k_cache, v_cache = _unpack_paged_kv_cache(paged_kv_cache, kv_layout)
    if append_key.dtype != k_cache.dtype or append_value.dtype != v_cache.dtype:
        raise ValueError("append_key/append_value dtype must match the cache dtype")
    if append_key.dim() != 3 or append_key.shape != append_value.shape:
        raise ValueError("append_key and append_value must be [nnz, num_kv_heads, head_dim]")
    dev = k_cache.device
    kv_indices = kv_indices.to(device=dev, dtype=torch.int32).contiguous()
    kv_indptr = kv_indptr.to(device=dev, dtype=torch.int32).contiguous()
    kv, _, num_kv_heads, head_dim = paged_kv(k_cache, v_cache, kv_layout, kv_indptr, kv_indices, None,
                                             kv_indptr.numel() - 1)
    if append_key.shape[1] != num_kv_heads or append_key.shape[2] != head_dim:
        raise ValueError("append_key shape does not match the cache")
    if append_key.stride(-1) != 1:
        append_key = append_key.contiguous()
    if append_value.stride(-1) != 1:
        append_value = append_value.contiguous()
    batch_indices = batch_indices.to(device=dev, dtype=torch.int32).contiguous()
    positions = positions.to(device=dev, dtype=torch.int32).contiguous()
    nnz = append_key.shape[0]
    if batch_indices.numel() != nnz or positions.numel() != nnz:
        raise ValueError("batch_indices and positions must have nnz entries")
    with torch.cuda.device(dev):
        _lib.check(
            _lib.lib().fi_append_paged_kv_cache(
                append_key.data_ptr(), append_value.data_ptr(), append_key.stride(0), append_key.stride(1),
                append_value.stride(0), append_value.stride(1), batch_indices.data_ptr(), positions.data_ptr(),
                nnz, C.byref(kv), _lib.current_stream(dev),
            ),
            "append_paged_kv_cache",
        )


def apply_rope_append_paged_kv_cache(
    q: torch.Tensor,
    append_key: torch.Tensor,
    append_value: torch.Tensor,
    batch_indices: torch.Tensor,
    positions: torch.Tensor,
    paged_kv_cache: Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]],
    kv_indices: torch.Tensor,
    kv_indptr: torch.Tensor,
    kv_last_page_len: torch.Tensor,
    kv_layout: str = "NHD",
    rotary_dim: Optional[int] = None,
    interleave: bool = False,
    rope_scale: float = 1,
    rope_theta: float = 1e4,
    pos_ids: Optional[torch.Tensor] = None,
    q_out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    r"""RoPE fused with the cache append: ``apply_rope_pos_ids(q, append_key, pos_ids)`` followed by
    ``append_paged_kv_cache(k_rope, append_value, ...)`` in one kernel -- every rotated key row is written once,
    straight into its page, instead of out to a temporary and back in (the serving-loop step right before the
    attention path).  Returns the rotated queries (``q_out`` if given; pass ``q_out=q`` for
    in place).  ``pos_ids`` defaults to ``positions`` (the row's position in its sequence); the cache must have the
    dtype of ``append_key``.  Bit-identical to the two calls it replaces.
    (ref: flashinfer/rope.py:321-420 apply_rope_pos_ids, flashinfer/page.py:299-425 append_paged_kv_cache)"""
    _check_kv_layout(kv_layout)
    for t, name in ((q, "q"), (append_key, "append_key"), (append_value, "append_value")):
        _lib.require_gpu_tensor(t, name)
    k_cache, v_cache = _unpack_paged_kv_cache(paged_kv_cache, kv_layout)
    if append_key.dtype != k_cache.dtype or append_value.dtype != v_cache.dtype or q.dtype != append_key.dtype:
        raise ValueError("q / append_key / append_value dtype must match the cache dtype")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("q and append_key must be float16 or bfloat16")
    if append_key.dim() != 3 or append_key.shape != append_value.shape or q.dim() != 3:
        raise ValueError("q, append_key and append_value must be [nnz, heads, head_dim]")
    dev = k_cache.device
    kv_indices = kv_indices.to(device=dev, dtype=torch.int32).contiguous()
    kv_indptr = kv_indptr.to(device=dev, dtype=torch.int32).contiguous()
    kv, _, num_kv_heads, head_dim = paged_kv(k_cache, v_cache, kv_layout, kv_indptr, kv_indices, None,
                                             kv_indptr.numel() - 1)
    if append_key.shape[1] != num_kv_heads or append_key.shape[2] != head_dim or q.shape[2] != head_dim or \
            q.shape[0] != append_key.shape[0]:
        raise ValueError("q / append_key shape does not match the cache")
    if q.stride(-1) != 1:
        q = q.contiguous()
    if append_key.stride(-1) != 1:
        append_key = append_key.contiguous()
    if append_value.stride(-1) != 1:
        append_value = append_value.contiguous()
    if q_out is None:
        q_out = torch.empty_like(q)
    elif q_out.shape != q.shape or q_out.dtype != q.dtype or q_out.stride(-1) != 1:
        raise ValueError("q_out must match q")
    batch_indices = batch_indices.to(device=dev, dtype=torch.int32).contiguous()
    positions = positions.to(device=dev, dtype=torch.int32).contiguous()
    pos_ids = positions if pos_ids is None else pos_ids.to(device=dev, dtype=torch.int32).contiguous()
    nnz = append_key.shape[0]
    if batch_indices.numel() != nnz or positions.numel() != nnz or pos_ids.numel() != nnz:
        raise ValueError("batch_indices, positions and pos_ids must have nnz entries")
    params = _lib.fi_rope_params_t(
        q=q.data_ptr(), k=append_key.data_ptr(), q_out=q_out.data_ptr(), k_out=None, pos_ids=pos_ids.data_ptr(),
        cos_sin_cache=None, q_stride_n=q.stride(0), q_stride_h=q.stride(1), k_stride_n=append_key.stride(0),
        k_stride_h=append_key.stride(1), qo_stride_n=q_out.stride(0), qo_stride_h=q_out.stride(1), ko_stride_n=0,
        ko_stride_h=0, nnz=nnz, num_q_heads=q.shape[1], num_k_heads=num_kv_heads, head_dim=head_dim,
        rotary_dim=head_dim if rotary_dim is None else rotary_dim, interleave=int(interleave),
        dtype=_lib.fi_dtype(q.dtype), rope_rcp_scale=1.0 / rope_scale, rope_rcp_theta=1.0 / rope_theta,
        smooth_a=0.0, smooth_b=0.0,
    )
    with torch.cuda.device(dev):
        _lib.check(
            _lib.lib().fi_apply_rope_append_paged_kv_cache(
                C.byref(params), append_value.data_ptr(), append_value.stride(0), append_value.stride(1),
                batch_indices.data_ptr(), positions.data_ptr(), C.byref(kv), _lib.current_stream(dev),
            ),
            "apply_rope_append_paged_kv_cache",
        )
    return q_out


def append_paged_mla_kv_cache(
    append_ckv: torch.Tensor,
    append_kpe: torch.Tensor,
    batch_indices: torch.Tensor,
    positions: torch.Tensor,
    ckv_cache: Optional[torch.Tensor],
    kpe_cache: Optional[torch.Tensor],
    kv_indices: torch.Tensor,
    kv_indptr: torch.Tensor,
    kv_last_page_len: torch.Tensor,
) -> None:
    r"""Append MLA rows to the paged ``ckv`` / ``kpe`` caches (in place; ref: flashinfer/page.py:250-298).

    append_ckv ``[nnz, 512]``, append_kpe ``[nnz, 64]`` (last dim contiguous); ckv_cache
    ``[num_pages, page_size, 512]``, kpe_cache ``[num_pages, page_size, 64]``; batch_indices / positions
    ``[nnz]`` int32 (see :func:`get_batch_indices_positions`); the page table is the one AFTER the append.
    Only ``ckv_dim = 512`` and ``kpe_dim = 64``; float16, bfloat16, float8_e4m3fn or float8_e5m2, one dtype for all
    four tensors (the rows are copied as they are: an fp8 cache takes the fp8 rows
    :func:`flashinfer.rope.mla_rope_quantize_fp8` returns).  Every row starts at a 16-byte boundary: strides are
    multiples of 8 elements at 16 bit and of 16 elements for fp8.
    """
    if ckv_cache is None or kpe_cache is None:
        raise ValueError("append_paged_mla_kv_cache: ckv_cache and kpe_cache are required")
    for t, name in ((append_ckv, "append_ckv"), (append_kpe, "append_kpe"), (ckv_cache, "ckv_cache"),
                    (kpe_cache, "kpe_cache")):
        _lib.require_gpu_tensor(t, name)
        if t.stride(-1) != 1:
            raise ValueError(f"append_paged_mla_kv_cache: {name} must have a contiguous last dimension")
    if ckv_cache.dim() == 4:
        ckv_cache = ckv_cache.squeeze(2)
    if kpe_cache.dim() == 4:
        kpe_cache = kpe_cache.squeeze(2)
    if append_ckv.dim() != 2 or append_kpe.dim() != 2 or append_ckv.shape[0] != append_kpe.shape[0]:
        raise ValueError("append_paged_mla_kv_cache: append_ckv / append_kpe must be [nnz, 512] / [nnz, 64]")
    if ckv_cache.dim() != 3 or kpe_cache.dim() != 3 or ckv_cache.shape[:2] != kpe_cache.shape[:2]:
        raise ValueError("append_paged_mla_kv_cache: caches must be [num_pages, page_size, dim]")
    if not (append_ckv.dtype == append_kpe.dtype == ckv_cache.dtype == kpe_cache.dtype):
        raise ValueError("append_paged_mla_kv_cache: all tensors must have one dtype")
    if append_ckv.shape[1] != ckv_cache.shape[2] or append_kpe.shape[1] != kpe_cache.shape[2]:
        raise ValueError("append_paged_mla_kv_cache: append rows do not match the cache width")
    dev = ckv_cache.device
    nnz = append_ckv.shape[0]
    batch_indices = batch_indices.to(device=dev, dtype=torch.int32).contiguous()
    positions = positions.to(device=dev, dtype=torch.int32).contiguous()
    kv_indices = kv_indices.to(device=dev, dtype=torch.int32).contiguous()
    kv_indptr = kv_indptr.to(device=dev, dtype=torch.int32).contiguous()
    if batch_indices.numel() != nnz or positions.numel() != nnz:
        raise ValueError("batch_indices and positions must have nnz entries")
    p = _lib.fi_append_paged_mla_kv_params_t(
        append_ckv=append_ckv.data_ptr(), append_ckv_stride_n=append_ckv.stride(0),
        append_kpe=append_kpe.data_ptr(), append_kpe_stride_n=append_kpe.stride(0),
        batch_indices=batch_indices.data_ptr(), positions=positions.data_ptr(),
        ckv_cache=ckv_cache.data_ptr(), ckv_stride_page=ckv_cache.stride(0), ckv_stride_n=ckv_cache.stride(1),
        kpe_cache=kpe_cache.data_ptr(), kpe_stride_page=kpe_cache.stride(0), kpe_stride_n=kpe_cache.stride(1),
        kv_indices=kv_indices.data_ptr(), kv_indptr=kv_indptr.data_ptr(), nnz=nnz, page_size=ckv_cache.shape[1],
        head_dim_ckv=ckv_cache.shape[2], head_dim_kpe=kpe_cache.shape[2], dtype=_lib.fi_dtype(ckv_cache.dtype),
    )
    with torch.cuda.device(dev):
        _lib.check(
            _lib.lib().fi_append_paged_mla_kv_cache(C.byref(p), _lib.current_stream(dev)),
            "append_paged_mla_kv_cache",
        )
