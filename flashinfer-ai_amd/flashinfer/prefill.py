"""Prefill / append attention operators: ``single_prefill_with_kv_cache`` and
``BatchPrefillWithPagedKVCacheWrapper`` (plan / run split).

Same names, arguments and defaults as the reference's ``flashinfer/prefill.py`` (single :960-1194;
wrapper :1226-2238).  The kernels are csrc/prefill_kernel.h (MFMA flash attention, GQA-packed tiles);
there is one backend, so ``backend`` accepts ``auto`` / ``fa2`` / ``fa3`` and means the same thing.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Any, List, Optional, Tuple, Union

import torch

from . import _lib
from ._plan_free import (_check_block_tables_and_lens, _check_len_fits_block_tables, _device_plan_regions,
                         _hnd_cache_views, _one_sinks_tensor, _out_or_empty, _refuse_fp4_out_and_shared_kv)
from ._wrapper import BatchAttentionWrapper
from .page import get_seq_lens
from .quantization import packbits, segment_packbits
from .utils import (
    MaskMode,
    PosEncodingMode,
    _apply_v_scale,
    _check_cached_qkv_data_type,
    _check_kv_layout,
    _check_pos_encoding_mode,
    _get_cache_alibi_slopes_buf,
    _get_cache_buf,
    _resolve_logits_params,
    _unpack_paged_kv_cache,
    canonicalize_qkv_dtypes,
    canonicalize_torch_dtype,
    check_shape_dtype_device,
    dense_kv_dims,
    is_float8,
    paged_kv,
    ragged_kv,
)


def _scale_tensor(x, n: int, device) -> Optional[torch.Tensor]:
    """per-head fp8 scale as a float32 device tensor of n entries (None stays None)."""
    if x is None:
        return None
    if not torch.is_tensor(x):
        # created on the device: no pageable host-to-device copy (which would sync, and fail under capture)
        return torch.full((n,), float(x), dtype=torch.float32, device=device)
    x = x.to(device=device, dtype=torch.float32).contiguous()
    if x.numel() == 1 and n != 1:
        x = x.expand(n).contiguous()
    if x.numel() != n:
        raise ValueError(f"scale tensor must have {n} entries, got {x.numel()}")
    return x


def _check_multi_item_args(prefix_len_ptr, token_pos_in_items_ptr, max_item_len_ptr, token_pos_in_items_len,
                           batch_size, device):
    """multi-item scoring operands (ref: flashinfer/prefill.py:1547-1558): uint32 prefix lengths, uint16 token
    positions (row stride token_pos_in_items_len), uint16 max item lengths (optional here: only used by the
    reference to skip masked tiles)."""
    if prefix_len_ptr is None and token_pos_in_items_ptr is None and max_item_len_ptr is None:
        return None, None, None, 0
    if prefix_len_ptr is None or token_pos_in_items_ptr is None:
        raise ValueError("multi-item scoring needs prefix_len_ptr and token_pos_in_items_ptr")
    if prefix_len_ptr.dtype != torch.uint32 or token_pos_in_items_ptr.dtype != torch.uint16:
        raise ValueError("prefix_len_ptr must be uint32 and token_pos_in_items_ptr uint16")
    if max_item_len_ptr is not None and max_item_len_ptr.dtype != torch.uint16:
        raise ValueError("max_item_len_ptr must be uint16")
    if prefix_len_ptr.numel() != batch_size:
        raise ValueError("prefix_len_ptr must have one entry per request")
    if token_pos_in_items_len <= 0 or token_pos_in_items_ptr.numel() < batch_size * token_pos_in_items_len:
        raise ValueError("token_pos_in_items_ptr is shorter than batch_size rows of token_pos_in_items_len")
    return (prefix_len_ptr.to(device).contiguous(), token_pos_in_items_ptr.to(device).contiguous(),
            None if max_item_len_ptr is None else max_item_len_ptr.to(device).contiguous(), int(token_pos_in_items_len))


def _check_multi_item_rows(prefix_len_ptr, token_pos_in_items_len, kv_lens_host):
    """The kernel reads token_pos_in_items[b][q_pos - prefix_len[b]] for every query position past the prefix, i.e. up
    to kv_len[b] - prefix_len[b] entries of row b: a shorter row would read the next request's row (or past the
    buffer) and the mask would be silently wrong.  plan() holds the kv lengths on the host; the prefix lengths come
    back with one small copy (plan() is synchronous host code anyway, ref: prefill.py:1547-1558)."""
    if prefix_len_ptr is None:
        return
    prefix = prefix_len_ptr.to("cpu").to(torch.int64)
    need = kv_lens_host.to(torch.int64) - prefix
    if bool((need > token_pos_in_items_len).any()):
        b = int(torch.nonzero(need > token_pos_in_items_len)[0])
        raise ValueError(
            f"multi-item scoring: request {b} has kv_len - prefix_len = {int(need[b])} positions past its prefix but "
            f"token_pos_in_items_len is {token_pos_in_items_len}")


def _mask_mode(wrapper) -> int:
    # ref: flashinfer/prefill.py:2091-2100
    if wrapper._custom_mask_buf is not None:
        return MaskMode.CUSTOM.value
    if wrapper._prefix_len_ptr is not None:
        return MaskMode.MULTIITEMSCORING.value
    return MaskMode.CAUSAL.value if wrapper._causal else MaskMode.NON_CAUSAL.value


def _plan_custom_mask(wrapper, custom_mask, packed_custom_mask, qo_indptr_host, kv_lens_host, non_blocking):
    """(packed mask, byte indptr) on the wrapper's device, or (None, None).
    ref: _compute_page_mask_indptr + segment_packbits, flashinfer/prefill.py:1203-1223, 1693-1706; in
    CUDA-graph mode the caller-provided custom_mask_buf / mask_indptr_buf are filled (:1838-1857)."""
    if custom_mask is None and packed_custom_mask is None:
        return None, None
    qo_lens = (qo_indptr_host[1:] - qo_indptr_host[:-1]).to(torch.int64)
    bits = qo_lens * kv_lens_host.to(torch.int64)
    bit_indptr = torch.zeros(len(qo_indptr_host), dtype=torch.int64)
    bit_indptr[1:] = torch.cumsum(bits, 0)
    if int(((bits + 7) // 8).sum()) >= 2 ** 31:
        raise ValueError("custom mask too large: byte offsets must fit int32")
    if packed_custom_mask is None:
        custom_mask = custom_mask.to(wrapper.device).contiguous().view(-1)
        if custom_mask.numel() != int(bit_indptr[-1]):
            raise ValueError(
                f"custom_mask has {custom_mask.numel()} entries, expected sum(qo_len * kv_len) = {int(bit_indptr[-1])}")
        packed_custom_mask, mask_indptr = segment_packbits(
            custom_mask, bit_indptr.to(torch.int32).to(wrapper.device), bitorder="little")
    else:
        mask_indptr = torch.zeros(len(qo_indptr_host), dtype=torch.int32)
        mask_indptr[1:] = torch.cumsum((bits + 7) // 8, 0)
        mask_indptr = mask_indptr.to(wrapper.device, non_blocking=non_blocking)
        packed_custom_mask = packed_custom_mask.to(wrapper.device)
        if packed_custom_mask.dtype != torch.uint8:
            raise ValueError("packed_custom_mask must be uint8")
    if wrapper.is_cuda_graph_enabled:
        mask_buf, indptr_buf = wrapper._user_custom_mask_buf, wrapper._user_mask_indptr_buf
        if mask_buf is None or indptr_buf is None:
            raise ValueError("custom_mask_buf and mask_indptr_buf are required for custom masks in cuda graph mode")
        if packed_custom_mask.numel() > mask_buf.numel():
            raise ValueError("packed custom mask exceeds custom_mask_buf")
        mask_buf[: packed_custom_mask.numel()].copy_(packed_custom_mask, non_blocking=non_blocking)
        indptr_buf[: len(mask_indptr)].copy_(mask_indptr, non_blocking=non_blocking)
        return mask_buf, indptr_buf
    return packed_custom_mask.contiguous(), mask_indptr.contiguous()


def _out_and_lse(q, out, lse, return_lse, out_shape, o_dtype):
    """``out`` (allocated, or checked to be ``out_shape`` / ``o_dtype`` on q's device) and, with ``return_lse``, the
    ``[rows, num_qo_heads]`` float32 ``lse`` (likewise); ``lse`` is None without ``return_lse``."""
    if return_lse:
        if lse is None:
            lse = torch.empty((q.size(0), q.size(1)), dtype=torch.float32, device=q.device)
        else:
            check_shape_dtype_device(lse, (q.size(0), q.size(1)), torch.float32, q.device, "lse")
    else:
        lse = None
    if out is None:
        out = torch.empty(out_shape, dtype=o_dtype, device=q.device)
    else:
        check_shape_dtype_device(out, out_shape, o_dtype, q.device, "out")
    return out, lse


def _run_single_prefill(run_fn, params, device):
    """``run_fn`` (fi_single_prefill_run or fi_single_prefill_qkvo_run) with the cached scratch buffer for split-KV
    partial states (ref: the 32 MB cached buffer of single_prefill, prefill.py:1125)."""
    tmp = _get_cache_buf("single_prefill_with_kv_cache_tmp", 32 * 1024 * 1024, device)
    with torch.cuda.device(device):
        _lib.check(
            run_fn(C.byref(params), tmp.data_ptr(), _lib.nbytes(tmp), _lib.current_stream(device)),
            "single_prefill_with_kv_cache",
        )


def _run_batch_prefill(wrapper, name, q, kv, o_dtype, out, lse, return_lse, window_left, q_scale, k_scale, v_scale,
                       scale_q=None, scale_k=None, scale_v=None, sinks=None, sm_scale=None):
    """run() of the paged and ragged wrappers once the kv view ``kv`` (a ``_lib.fi_paged_kv_t``; ragged: an identity
    table of one-token pages) is resolved and checked against the plan: out / lse, fi_batch_prefill_paged_run, v_scale.
    ``sinks``: the per-head attention sinks (then fi_batch_prefill_paged_run_sinks); ``sm_scale``: a softmax scale
    given to this run() in place of the planned one (the AttentionSink call form)."""
    sinks_ptr = wrapper._sinks_ptr(sinks, q)
    if q.stride(-1) != 1:
        q = q.contiguous()
    out, lse = _out_and_lse(q, out, lse, return_lse, q.shape[:-1] + (kv.head_dim,), o_dtype)
    alibi = _get_cache_alibi_slopes_buf(q.shape[1], q.device) if wrapper._pos_encoding_mode == "ALIBI" else None
    params = _lib.fi_batch_prefill_params_t(
        q=q.data_ptr(), q_stride_n=q.stride(0), q_stride_h=q.stride(1), qo_indptr=wrapper._qo_indptr_buf.data_ptr(),
        kv=kv, o=out.data_ptr(), lse=_lib.ptr(lse), alibi_slopes=_lib.ptr(alibi),
        scale_q=_lib.ptr(scale_q), scale_k=_lib.ptr(scale_k), scale_v=_lib.ptr(scale_v),
        num_qo_heads=wrapper._num_qo_heads, q_dtype=_lib.fi_dtype(q.dtype), o_dtype=_lib.fi_dtype(o_dtype),
        custom_mask=_lib.ptr(wrapper._custom_mask_buf), mask_indptr=_lib.ptr(wrapper._mask_indptr_buf),
        prefix_len_ptr=_lib.ptr(wrapper._prefix_len_ptr),
        token_pos_in_items_ptr=_lib.ptr(wrapper._token_pos_in_items_ptr),
        max_item_len_ptr=_lib.ptr(wrapper._max_item_len_ptr), token_pos_in_items_len=wrapper._token_pos_in_items_len,
        mask_mode=_mask_mode(wrapper), pos_encoding_mode=PosEncodingMode[wrapper._pos_encoding_mode].value,
        window_left=window_left, bf16_pv_mode=wrapper._bf16_pv_mode,
        **_resolve_logits_params(q.size(-1), wrapper._sm_scale if sm_scale is None else sm_scale, q_scale, k_scale,
                                 wrapper._logits_soft_cap, wrapper._rope_scale, wrapper._rope_theta),
    )
    with torch.cuda.device(q.device):
        plan_and_params = (wrapper._plan_info, _lib.FI_PREFILL_PLAN_INFO_LEN, C.byref(params))
        if sinks_ptr:
            status = _lib.lib().fi_batch_prefill_paged_run_sinks(
                *wrapper._workspace_args, *plan_and_params, sinks_ptr, _lib.current_stream(q.device))
        else:
            status = _lib.lib().fi_batch_prefill_paged_run(
                *wrapper._workspace_args, *plan_and_params, _lib.current_stream(q.device))
        _lib.check(status, name)
    if v_scale is not None:
        out = _apply_v_scale(out, v_scale)
    return (out, lse) if return_lse else out


# Unequal (head_dim_qk, head_dim_vo) pairs with a kernel of their own (csrc/prefill_qkvo_kernel.h): DeepSeek-style MLA
# prefill in its non-absorbed form, 128 nope + 64 rope dims for q / k and 128-dim v (ref: aot.py:568).
_QKVO_HEAD_DIMS = ((192, 128),)


def _check_qkvo_config(head_dim_qk, head_dim_vo, q_dtype, kv_dtype, pos_encoding_mode, logits_soft_cap, masked):
    """ValueError for whatever the head_dim_qk 192 / head_dim_vo 128 kernel does not run."""
    if (head_dim_qk, head_dim_vo) not in _QKVO_HEAD_DIMS:
        raise ValueError(f"head_dim_qk {head_dim_qk} / head_dim_vo {head_dim_vo} is unsupported: the head dims must be "
                         "equal, or 192 / 128")
    if q_dtype not in (torch.float16, torch.bfloat16) or kv_dtype != q_dtype:
        raise ValueError(f"head_dim_qk {head_dim_qk} / head_dim_vo {head_dim_vo} needs float16 or bfloat16 q and kv "
                         f"of one dtype (got {q_dtype} / {kv_dtype}; there is no fp8 kernel for this pair)")
    if pos_encoding_mode != "NONE":
        raise ValueError(f"head_dim_qk {head_dim_qk} / head_dim_vo {head_dim_vo} supports pos_encoding_mode='NONE' "
                         f"only (got {pos_encoding_mode!r}): apply RoPE to the rope dims before the call")
    if logits_soft_cap:
        raise ValueError(f"head_dim_qk {head_dim_qk} / head_dim_vo {head_dim_vo} does not support logits_soft_cap")
    if masked:
        raise ValueError(f"head_dim_qk {head_dim_qk} / head_dim_vo {head_dim_vo} does not support custom masks or "
                         "multi-item scoring (causal / non-causal and window_left only)")


def _qkvo_params(q, k, v, kv_layout, out, lse, causal, window_left, sm_scale, bf16_pv_mode, **extra):
    """fi_prefill_qkvo_params_t for q [rows, Hq, 192] and k / v [kv rows, Hkv, 192 / 128] (NHD; HND: heads first),
    k and v each by their own strides."""
    _, num_kv_heads, k_sn, k_sh = dense_kv_dims(k, kv_layout)
    _, _, v_sn, v_sh = dense_kv_dims(v, kv_layout)
    dt = _lib.fi_dtype(q.dtype)
    return _lib.fi_prefill_qkvo_params_t(
        q=q.data_ptr(), q_stride_n=q.stride(0), q_stride_h=q.stride(1), k=k.data_ptr(), k_stride_n=k_sn,
        k_stride_h=k_sh, v=v.data_ptr(), v_stride_n=v_sn, v_stride_h=v_sh, o=out.data_ptr(), lse=_lib.ptr(lse),
        num_qo_heads=q.shape[1], num_kv_heads=num_kv_heads,
        head_dim_qk=q.shape[2], head_dim_vo=v.shape[2], q_dtype=dt, kv_dtype=_lib.fi_dtype(k.dtype), o_dtype=dt,
        mask_mode=MaskMode.CAUSAL.value if causal else MaskMode.NON_CAUSAL.value,
        pos_encoding_mode=PosEncodingMode.NONE.value, window_left=window_left, logits_soft_cap=0.0,
        sm_scale=sm_scale, bf16_pv_mode=bf16_pv_mode, **extra,
    )


def _check_qkvo_kv(k, v):
    if k.dim() != 3 or v.dim() != 3 or k.stride(-1) != 1 or v.stride(-1) != 1:
        raise ValueError("k and v must be 3-D and contiguous in their last dim")


def _single_prefill_qkvo(q, k, v, causal, kv_layout, pos_encoding_mode, sm_scale, window_left, logits_soft_cap,
                         return_lse, bf16_pv_exact_range, masked, o_dtype):
    """single_prefill_with_kv_cache for v.shape[-1] != q.shape[-1] (head_dim_qk 192 / head_dim_vo 128)."""
    _check_qkvo_kv(k, v)
    head_dim_qk, head_dim_vo = q.shape[-1], v.shape[-1]
    _check_qkvo_config(head_dim_qk, head_dim_vo, q.dtype, k.dtype, pos_encoding_mode, logits_soft_cap, masked)
    if k.shape[:-1] != v.shape[:-1] or k.shape[-1] != head_dim_qk or v.dtype != k.dtype:
        raise ValueError("k must be [.., head_dim_qk] and v [.., head_dim_vo] over the same tokens and heads, one dtype")
    if o_dtype is not None and o_dtype != q.dtype:
        raise ValueError("the output dtype must equal the q dtype at head_dim_qk 192 / head_dim_vo 128")
    if q.stride(-1) != 1:
        q = q.contiguous()
    qo_len, num_qo_heads = q.shape[0], q.shape[1]
    kv_len = dense_kv_dims(k, kv_layout)[0]
    out, lse = _out_and_lse(q, None, None, return_lse, (qo_len, num_qo_heads, head_dim_vo), q.dtype)
    params = _qkvo_params(q, k, v, kv_layout, out, lse, causal, window_left,
                          1.0 / math.sqrt(head_dim_qk) if sm_scale is None else sm_scale,
                          1 if bf16_pv_exact_range else 0, qo_len=qo_len, kv_len=kv_len)
    _run_single_prefill(_lib.lib().fi_single_prefill_qkvo_run, params, q.device)
    return (out, lse) if return_lse else out


def single_prefill_with_kv_cache(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    scale_q: Optional[torch.Tensor] = None,
    scale_k: Optional[torch.Tensor] = None,
    scale_v: Optional[torch.Tensor] = None,
    o_dtype: Optional[torch.dtype] = None,
    custom_mask: Optional[torch.Tensor] = None,
    packed_custom_mask: Optional[torch.Tensor] = None,
    causal: bool = False,
    kv_layout: str = "NHD",
    pos_encoding_mode: str = "NONE",
    use_fp16_qk_reduction: bool = False,
    sm_scale: Optional[float] = None,
    window_left: int = -1,
    logits_soft_cap: Optional[float] = None,
    rope_scale: Optional[float] = None,
    rope_theta: Optional[float] = None,
    backend: str = "auto",
    return_lse: bool = False,
    bf16_pv_exact_range: bool = False,
) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    r"""Prefill / append attention with KV cache for a single request.

    Parameters
    ----------
    q : ``[qo_len, num_qo_heads, head_dim]``
    k, v : ``[kv_len, num_kv_heads, head_dim]`` (``NHD``) or ``[num_kv_heads, kv_len, head_dim]`` (``HND``)
    scale_q, scale_k, scale_v : per-head scales (``[num_qo_heads]`` / ``[num_kv_heads]``) for fp8 inputs
    o_dtype : output dtype (required for fp8 attention; defaults to ``q.dtype``)
    causal : apply the causal mask (query i sees keys up to ``i + kv_len - qo_len``)
    pos_encoding_mode : ``NONE`` / ``ROPE_LLAMA`` (applied in-kernel) / ``ALIBI``
    sm_scale, window_left, logits_soft_cap, rope_scale, rope_theta : as the reference
    return_lse : also return the base-2 logsumexp, shape ``[qo_len, num_qo_heads]``
    bf16_pv_exact_range : (extension, bf16 queries) ``True`` when ``v`` may hold ``|v| >= 65504`` or many
        ``|v| < 6e-5``: the kernel then keeps V in bf16 and enters P as hi + lo bf16 halves (about 25 % slower)
        instead of running P.V on the f16 matrix cores, whose V operand is exact only inside f16's normal range

    custom_mask : ``[qo_len, kv_len]`` bool; packed_custom_mask : its ``packbits(..., bitorder="little")``
        form (takes precedence).  With a mask, ``causal`` is ignored (mask mode CUSTOM).
    (ref: flashinfer/prefill.py:960-1194)
    """
    _check_pos_encoding_mode(pos_encoding_mode)
    _check_kv_layout(kv_layout)
    if custom_mask is not None and packed_custom_mask is None:
        # ref: prefill.py:1114-1118
        packed_custom_mask = packbits(custom_mask.contiguous().view(-1), bitorder="little")
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        _lib.require_gpu_tensor(t, name)
    if q.dim() == 3 and v.dim() == 3 and v.shape[-1] != q.shape[-1]:
        # head_dim_qk = q.shape[-1], head_dim_vo = v.shape[-1] (ref: prefill.py:1166-1167)
        return _single_prefill_qkvo(q, k, v, causal, kv_layout, pos_encoding_mode, sm_scale, window_left,
                                    logits_soft_cap, return_lse, bf16_pv_exact_range, packed_custom_mask is not None,
                                    o_dtype)
    if q.dim() != 3 or k.dim() != 3 or k.shape != v.shape:
        raise ValueError("q must be [qo_len, num_qo_heads, head_dim]; k, v 3-D with equal shapes")
    qo_len, num_qo_heads, head_dim = q.shape
    kv_len, num_kv_heads, stride_n, stride_h = dense_kv_dims(k, kv_layout)
    if k.stride() != v.stride() or k.stride(-1) != 1 or q.stride(-1) != 1:
        raise ValueError("k and v must share strides and q/k/v must be contiguous in head_dim")
    if is_float8(q):
        assert window_left == -1
        assert q.dtype == k.dtype == v.dtype
        # a missing scale is passed as NULL (= 1, include/fi_mi355.h): no tensor is created
        scale_q = _scale_tensor(scale_q, num_qo_heads, q.device)
        scale_k = _scale_tensor(scale_k, num_kv_heads, q.device)
        scale_v = _scale_tensor(scale_v, num_kv_heads, q.device)
        if o_dtype is None:
            raise ValueError("o_dtype should be provided for FP8 attention")
    else:
        scale_q = scale_k = scale_v = None
    if o_dtype is None:
        o_dtype = q.dtype
    out, lse = _out_and_lse(q, None, None, return_lse, q.shape[:-1] + v.shape[-1:], o_dtype)
    if packed_custom_mask is not None:
        _lib.require_gpu_tensor(packed_custom_mask, "packed_custom_mask")
        if packed_custom_mask.dtype != torch.uint8 or packed_custom_mask.numel() * 8 < qo_len * kv_len:
            raise ValueError("packed_custom_mask must be uint8 with at least qo_len * kv_len bits")
        packed_custom_mask = packed_custom_mask.contiguous()
    alibi = _get_cache_alibi_slopes_buf(num_qo_heads, q.device) if pos_encoding_mode == "ALIBI" else None
    params = _lib.fi_single_prefill_params_t(
        q=q.data_ptr(), q_stride_n=q.stride(0), q_stride_h=q.stride(1), k=k.data_ptr(), v=v.data_ptr(),
        kv_stride_n=stride_n, kv_stride_h=stride_h, o=out.data_ptr(), lse=_lib.ptr(lse),
        alibi_slopes=_lib.ptr(alibi), scale_q=_lib.ptr(scale_q), scale_k=_lib.ptr(scale_k),
        scale_v=_lib.ptr(scale_v), qo_len=qo_len, kv_len=kv_len, num_qo_heads=num_qo_heads,
        num_kv_heads=num_kv_heads, head_dim=head_dim, q_dtype=_lib.fi_dtype(q.dtype),
        kv_dtype=_lib.fi_dtype(k.dtype), o_dtype=_lib.fi_dtype(o_dtype),
        custom_mask=_lib.ptr(packed_custom_mask),
        mask_mode=(MaskMode.CUSTOM.value if packed_custom_mask is not None
                   else MaskMode.CAUSAL.value if causal else MaskMode.NON_CAUSAL.value),
        pos_encoding_mode=PosEncodingMode[pos_encoding_mode].value, window_left=window_left,
        bf16_pv_mode=1 if bf16_pv_exact_range else 0,
        **_resolve_logits_params(head_dim, sm_scale, None, None, logits_soft_cap, rope_scale, rope_theta),
    )
    _run_single_prefill(_lib.lib().fi_single_prefill_run, params, q.device)
    return (out, lse) if return_lse else out


single_prefill_with_kv_cache_return_lse = functools.partial(
    single_prefill_with_kv_cache, return_lse=True
)


class BatchPrefillWithPagedKVCacheWrapper(BatchAttentionWrapper):
    r"""Prefill / append attention over a paged KV cache for a batch of requests.

    >>> prefill_wrapper = flashinfer.BatchPrefillWithPagedKVCacheWrapper(workspace_buffer, "NHD")
    >>> prefill_wrapper.plan(qo_indptr, paged_kv_indptr, paged_kv_indices, paged_kv_last_page_len,
    ...                      num_qo_heads, num_kv_heads, head_dim, page_size, causal=True)
    >>> o = prefill_wrapper.run(q, kv_cache)          # [qo_indptr[-1], num_qo_heads, head_dim]

    (ref: flashinfer/prefill.py:1226-2238; example page table :1247-1259)
    """

    def __init__(
        self,
        float_workspace_buffer: torch.Tensor,
        kv_layout: str = "NHD",
        use_cuda_graph: bool = False,
        qo_indptr_buf: Optional[torch.Tensor] = None,
        paged_kv_indptr_buf: Optional[torch.Tensor] = None,
        paged_kv_indices_buf: Optional[torch.Tensor] = None,
        paged_kv_last_page_len_buf: Optional[torch.Tensor] = None,
        custom_mask_buf: Optional[torch.Tensor] = None,
        mask_indptr_buf: Optional[torch.Tensor] = None,
        backend: str = "auto",
        jit_args: Optional[List[Any]] = None,
        jit_kwargs: Optional[dict] = None,
    ) -> None:
        _check_kv_layout(kv_layout)
        # jit_args: None, or the reference's list for the "AttentionSink" variant (flashinfer/attention.py:241-255),
        # which makes run() take (q, paged_kv_cache, sink, sm_scale); jit_kwargs is accepted and unused
        super().__init__(float_workspace_buffer, use_cuda_graph, backend, ("auto", "fa2", "fa3"), jit_args,
                         sink_variant=True)
        self._kv_layout = kv_layout
        if use_cuda_graph:
            for buf, name in ((qo_indptr_buf, "qo_indptr_buf"), (paged_kv_indptr_buf, "paged_kv_indptr_buf"),
                              (paged_kv_indices_buf, "paged_kv_indices_buf"),
                              (paged_kv_last_page_len_buf, "paged_kv_last_page_len_buf")):
                if not torch.is_tensor(buf):
                    raise ValueError(f"{name} should be a torch.Tensor in CUDA graph mode")
            self._fixed_batch_size = len(qo_indptr_buf) - 1
            if len(paged_kv_indptr_buf) != self._fixed_batch_size + 1:
                raise ValueError("The length of paged_kv_indptr_buf should be batch_size + 1.")
            if len(paged_kv_last_page_len_buf) != self._fixed_batch_size:
                raise ValueError("The length of paged_kv_last_page_len_buf should be batch_size.")
        self._qo_indptr_buf = qo_indptr_buf
        self._paged_kv_indptr_buf = paged_kv_indptr_buf
        self._paged_kv_indices_buf = paged_kv_indices_buf
        self._paged_kv_last_page_len_buf = paged_kv_last_page_len_buf
        self._user_custom_mask_buf = custom_mask_buf
        self._user_mask_indptr_buf = mask_indptr_buf
        self._custom_mask_buf = self._mask_indptr_buf = None

    def plan(
        self,
        qo_indptr: torch.Tensor,
        paged_kv_indptr: torch.Tensor,
        paged_kv_indices: torch.Tensor,
        paged_kv_last_page_len: torch.Tensor,
        num_qo_heads: int,
        num_kv_heads: int,
        head_dim_qk: int,
        page_size: int,
        head_dim_vo: Optional[int] = None,
        custom_mask: Optional[torch.Tensor] = None,
        packed_custom_mask: Optional[torch.Tensor] = None,
        causal: bool = False,
        pos_encoding_mode: str = "NONE",
        use_fp16_qk_reduction: bool = False,
        sm_scale: Optional[float] = None,
        window_left: int = -1,
        logits_soft_cap: Optional[float] = None,
        rope_scale: Optional[float] = None,
        rope_theta: Optional[float] = None,
        q_data_type: Union[str, torch.dtype] = "float16",
        kv_data_type: Optional[Union[str, torch.dtype]] = None,
        non_blocking: bool = True,
        prefix_len_ptr: Optional[torch.Tensor] = None,
        token_pos_in_items_ptr: Optional[torch.Tensor] = None,
        token_pos_in_items_len: int = 0,
        max_item_len_ptr: Optional[torch.Tensor] = None,
        seq_lens: Optional[torch.Tensor] = None,
        seq_lens_q: Optional[torch.Tensor] = None,
        block_tables: Optional[torch.Tensor] = None,
        max_token_per_sequence: Optional[int] = None,
        max_sequence_kv: Optional[int] = None,
        fixed_split_size: Optional[int] = None,
        disable_split_kv: bool = False,
        o_data_type: Optional[Union[str, torch.dtype]] = None,
        bf16_pv_exact_range: bool = False,
    ) -> None:
        r"""Plan batch prefill/append attention for the given ragged queries and page table.

        qo_indptr : ``[batch_size + 1]`` int32; paged_kv_indptr / indices / last_page_len as in decode.
        causal, pos_encoding_mode, sm_scale, window_left, logits_soft_cap, rope_* configure the variant.
        q_data_type / kv_data_type : dtypes the run() tensors will have (fp8 e4m3 for both = fp8 attention).
        o_data_type : (extension) output dtype; defaults to the q dtype, or bfloat16 for fp8 queries.
        bf16_pv_exact_range : (extension, bf16 queries) the cache may hold ``|v| >= 65504`` or many ``|v| < 6e-5``:
            P.V then runs with hi + lo bf16 probabilities instead of on the f16 matrix cores (no range limit on V,
            about 25 % slower); see :func:`single_prefill_with_kv_cache`.
        custom_mask : flattened bool mask, request i contributes ``qo_len[i] * kv_len[i]`` entries
            (row-major ``[qo_len, kv_len]``); packed_custom_mask : its ``segment_packbits(..., "little")`` form.
            With a mask the mask mode is CUSTOM and ``causal`` is ignored (ref: prefill.py:1693-1706, 1890-1905).
        prefix_len_ptr (uint32 ``[batch]``), token_pos_in_items_ptr (uint16 ``[batch * token_pos_in_items_len]``),
        token_pos_in_items_len, max_item_len_ptr (uint16 ``[batch]``): multi-item scoring -- a query past the
        request's prefix sees the prefix and the tokens of its own item (mask mode MULTIITEMSCORING; plan with
        ``causal=True``; ref: prefill.py:1547-1558, 2099-2100, prefill.cuh:795-858).
        (ref: flashinfer/prefill.py:1523-1921)
        """
        self._bf16_pv_mode = 1 if bf16_pv_exact_range else 0
        self._prefix_len_ptr, self._token_pos_in_items_ptr, self._max_item_len_ptr, self._token_pos_in_items_len = \
            _check_multi_item_args(prefix_len_ptr, token_pos_in_items_ptr, max_item_len_ptr, token_pos_in_items_len,
                                   len(qo_indptr) - 1, self.device)
        _check_pos_encoding_mode(pos_encoding_mode)
        q_data_type, kv_data_type = canonicalize_qkv_dtypes(q_data_type, kv_data_type)
        if o_data_type is None:
            o_data_type = torch.bfloat16 if q_data_type in (torch.float8_e4m3fn, torch.float8_e5m2) else q_data_type
        o_data_type = canonicalize_torch_dtype(o_data_type)
        if logits_soft_cap is None:
            logits_soft_cap = 0.0
        if head_dim_vo is None:
            head_dim_vo = head_dim_qk
        if head_dim_vo != head_dim_qk:
            # K and V share one page layout (ref: the paged wrappers take one head_dim)
            raise ValueError(f"the paged KV cache needs head_dim_qk == head_dim_vo (got {head_dim_qk} / {head_dim_vo}); "
                             "use BatchPrefillWithRaggedKVCacheWrapper for head_dim_qk 192 / head_dim_vo 128")
        batch_size = len(qo_indptr) - 1
        if len(paged_kv_indptr) != batch_size + 1 or len(paged_kv_last_page_len) != batch_size:
            raise ValueError("qo_indptr, paged_kv_indptr and paged_kv_last_page_len disagree on the batch size")

        qo_indptr_host = qo_indptr.to("cpu").contiguous()
        paged_kv_indptr_host = paged_kv_indptr.to("cpu").contiguous()
        paged_kv_last_page_len_host = paged_kv_last_page_len.to("cpu")
        if seq_lens is None:
            kv_lens_arr_host = get_seq_lens(paged_kv_indptr_host, paged_kv_last_page_len_host, page_size)
        else:
            kv_lens_arr_host = seq_lens.cpu()
        kv_lens_arr_host = kv_lens_arr_host.to(torch.int32).contiguous()
        _check_multi_item_rows(self._prefix_len_ptr, self._token_pos_in_items_len, kv_lens_arr_host)
        total_num_rows = int(qo_indptr_host[-1])
        self._custom_mask_buf, self._mask_indptr_buf = _plan_custom_mask(
            self, custom_mask, packed_custom_mask, qo_indptr_host, kv_lens_arr_host, non_blocking)
        if self._custom_mask_buf is not None:
            causal = False  # mask mode CUSTOM: every kv tile is visited, the bits decide

        self._bind_index_tensors(batch_size, non_blocking, prefix=("paged_kv_indices",), qo_indptr=qo_indptr,
                                 paged_kv_indptr=paged_kv_indptr, paged_kv_indices=paged_kv_indices,
                                 paged_kv_last_page_len=paged_kv_last_page_len)
        total_rows_bound = total_num_rows
        if self._use_cuda_graph and max_token_per_sequence is not None:
            total_rows_bound = max_token_per_sequence * batch_size
        self._plan_info = _lib.batch_prefill_plan(
            self._float_workspace_buffer, self._int_workspace_buffer, self._pin_memory_int_workspace_buffer,
            qo_indptr_host, paged_kv_indptr_host, kv_lens_arr_host, total_rows_bound, batch_size, num_qo_heads,
            num_kv_heads, page_size, self._use_cuda_graph, head_dim_qk, head_dim_vo, causal, window_left,
            -1 if fixed_split_size is None else fixed_split_size, disable_split_kv,
            "BatchPrefillWithPagedKVCacheWrapper.plan")
        self._batch_size = batch_size
        self._num_qo_heads = num_qo_heads
        self._num_kv_heads = num_kv_heads
        self._head_dim = head_dim_qk
        self._page_size = page_size
        self._total_num_rows = total_num_rows
        self._cached_q_data_type = q_data_type
        self._cached_kv_data_type = kv_data_type
        self._cached_o_data_type = o_data_type
        self._causal = causal
        self._set_run_options(pos_encoding_mode, window_left, logits_soft_cap, sm_scale, rope_scale, rope_theta)

    begin_forward = plan

    def forward(self, q, paged_kv_cache, causal=False, pos_encoding_mode="NONE", use_fp16_qk_reduction=False,
                k_scale=None, v_scale=None, window_left=-1, logits_soft_cap=None, sm_scale=None,
                rope_scale=None, rope_theta=None) -> torch.Tensor:
        r"""Warning: This function is deprecated, please use :meth:`run` instead."""
        self._causal = causal
        self._set_run_options(pos_encoding_mode, window_left, logits_soft_cap, sm_scale, rope_scale, rope_theta)
        return self.run(q, paged_kv_cache, k_scale=k_scale, v_scale=v_scale)

    def run(
        self,
        q: torch.Tensor,
        paged_kv_cache: Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]],
        *args,
        q_scale: Optional[float] = None,
        k_scale: Optional[float] = None,
        v_scale: Optional[float] = None,
        out: Optional[torch.Tensor] = None,
        lse: Optional[torch.Tensor] = None,
        return_lse: bool = False,
        enable_pdl: Optional[bool] = None,
        window_left: Optional[int] = None,
        sinks: Optional[torch.Tensor] = None,
        scale_q: Optional[torch.Tensor] = None,
        scale_k: Optional[torch.Tensor] = None,
        scale_v: Optional[torch.Tensor] = None,
    ) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        r"""Compute batch prefill/append attention between ``q`` and the paged KV cache.

        q : ``[qo_indptr[-1], num_qo_heads, head_dim]``; paged_kv_cache as in decode.
        q_scale / k_scale / v_scale : scalar calibration scales (folded into sm_scale / the output).
        scale_q / scale_k / scale_v : (extension) per-head fp8 scales ``[num_qo_heads]`` / ``[num_kv_heads]``
            for fp8 attention (the reference's FA3 kernel takes them, csrc/batch_prefill_fp8_sm90.cu:81-185,
            but its wrapper passes None).
        sinks : optional float32 ``[num_qo_heads]`` on the wrapper's device, contiguous: one attention-sink logit per
            head (natural-log units, not multiplied by ``sm_scale``) that joins the softmax denominator of every query
            row without a value vector (ref: flashinfer/jit/attention/variants.py:17-53); float16 / bfloat16 queries
            only.  ``-inf`` switches a head's sink off.  The returned logsumexp includes the sink, so a state with a
            folded sink must not be merged again (``merge_state`` and the cascade wrappers would count it twice).
        A wrapper built with the reference's "AttentionSink" ``jit_args`` is called as
        ``run(q, paged_kv_cache, sink, sm_scale)``.
        Returns ``[qo_indptr[-1], num_qo_heads, head_dim]`` (+ base-2 logsumexp ``[nnz, num_qo_heads]``).
        (ref: flashinfer/prefill.py:1979-2206)
        """
        args, sinks, sm_scale = self._sink_variant_args(args, sinks)
        self._check_run_args(args)
        _lib.require_gpu_tensor(q, "q")
        k_cache, v_cache = _unpack_paged_kv_cache(paged_kv_cache, self._kv_layout)
        _check_cached_qkv_data_type(q, k_cache, self._cached_q_data_type, self._cached_kv_data_type)
        kv, page_size, num_kv_heads, head_dim = paged_kv(
            k_cache, v_cache, self._kv_layout, self._paged_kv_indptr_buf, self._paged_kv_indices_buf,
            self._paged_kv_last_page_len_buf, self._batch_size)
        window_left = self._window_left if window_left is None else window_left
        assert window_left == self._window_left
        if q.dim() != 3 or q.shape[0] != self._total_num_rows or q.shape[1] != self._num_qo_heads:
            raise ValueError(
                f"q must have shape [{self._total_num_rows}, {self._num_qo_heads}, head_dim], got {tuple(q.shape)}"
            )
        if q.shape[2] != head_dim or head_dim != self._head_dim:
            raise ValueError("head_dim of q / kv cache does not match the planned head_dim")
        if num_kv_heads != self._num_kv_heads or page_size != self._page_size:
            raise ValueError("kv cache shape does not match the planned num_kv_heads / page_size")
        if out is not None and not out.is_contiguous():
            raise ValueError("out must be contiguous")
        # missing scales are NULL pointers (= 1 in the kernels): run() creates no tensor and stays capturable
        return _run_batch_prefill(
            self, "BatchPrefillWithPagedKVCacheWrapper.run", q, kv, self._cached_o_data_type, out, lse, return_lse,
            window_left, q_scale, k_scale, v_scale, _scale_tensor(scale_q, self._num_qo_heads, q.device),
            _scale_tensor(scale_k, num_kv_heads, q.device), _scale_tensor(scale_v, num_kv_heads, q.device),
            sinks=sinks, sm_scale=sm_scale)

    run_return_lse = functools.partialmethod(run, return_lse=True)

    def forward_return_lse(self, q, paged_kv_cache, causal=False, pos_encoding_mode="NONE",
                           use_fp16_qk_reduction=False, k_scale=None, v_scale=None, window_left=-1,
                           logits_soft_cap=None, sm_scale=None, rope_scale=None, rope_theta=None):
        r"""Warning: This function is deprecated, please use :meth:`run_return_lse` instead."""
        self._causal = causal
        self._set_run_options(pos_encoding_mode, window_left, logits_soft_cap, sm_scale, rope_scale, rope_theta)
        return self.run_return_lse(q, paged_kv_cache, k_scale=k_scale, v_scale=v_scale)

    def end_forward(self) -> None:
        r"""Warning: this function is deprecated and has no effect."""
        pass


class BatchPrefillWithRaggedKVCacheWrapper(BatchAttentionWrapper):
    r"""Prefill / append attention with ragged (tensor) KV for a batch of requests: ``k``/``v`` are
    ``[kv_indptr[-1], num_kv_heads, head_dim]`` (``NHD``) or ``[num_kv_heads, kv_indptr[-1], head_dim]`` (``HND``).

    Runs the paged kernels with an identity page table of one-token pages (see include/fi_mi355.h).
    (ref: flashinfer/prefill.py:2255-3007)
    """

    def __init__(
        self,
        float_workspace_buffer: torch.Tensor,
        kv_layout: str = "NHD",
        use_cuda_graph: bool = False,
        qo_indptr_buf: Optional[torch.Tensor] = None,
        kv_indptr_buf: Optional[torch.Tensor] = None,
        custom_mask_buf: Optional[torch.Tensor] = None,
        mask_indptr_buf: Optional[torch.Tensor] = None,
        backend: str = "auto",
        jit_args: Optional[List[Any]] = None,
        jit_kwargs: Optional[dict] = None,
    ) -> None:
        _check_kv_layout(kv_layout)
        # jit_args: None, or the reference's "AttentionSink" list: run() is then run(q, k, v, sink, sm_scale)
        super().__init__(float_workspace_buffer, use_cuda_graph, backend, ("auto", "fa2", "fa3"), jit_args,
                         sink_variant=True)
        self._kv_layout = kv_layout
        if use_cuda_graph:
            if not torch.is_tensor(qo_indptr_buf) or not torch.is_tensor(kv_indptr_buf):
                raise ValueError("qo_indptr_buf and kv_indptr_buf should be torch.Tensor in cuda graph mode")
            self._fixed_batch_size = len(qo_indptr_buf) - 1
            if len(kv_indptr_buf) != self._fixed_batch_size + 1:
                raise ValueError("The length of kv_indptr_buf should be batch_size + 1.")
        self._qo_indptr_buf = qo_indptr_buf
        self._kv_indptr_buf = kv_indptr_buf
        self._user_custom_mask_buf = custom_mask_buf
        self._user_mask_indptr_buf = mask_indptr_buf
        self._custom_mask_buf = self._mask_indptr_buf = None

    def plan(
        self,
        qo_indptr: torch.Tensor,
        kv_indptr: torch.Tensor,
        num_qo_heads: int,
        num_kv_heads: int,
        head_dim_qk: int,
        head_dim_vo: Optional[int] = None,
        custom_mask: Optional[torch.Tensor] = None,
        packed_custom_mask: Optional[torch.Tensor] = None,
        causal: bool = False,
        pos_encoding_mode: str = "NONE",
        use_fp16_qk_reduction: bool = False,
        window_left: int = -1,
        logits_soft_cap: Optional[float] = None,
        sm_scale: Optional[float] = None,
        rope_scale: Optional[float] = None,
        rope_theta: Optional[float] = None,
        q_data_type: Union[str, torch.dtype] = "float16",
        kv_data_type: Optional[Union[str, torch.dtype]] = None,
        non_blocking: bool = True,
        prefix_len_ptr: Optional[torch.Tensor] = None,
        token_pos_in_items_ptr: Optional[torch.Tensor] = None,
        token_pos_in_items_len: int = 0,
        max_item_len_ptr: Optional[torch.Tensor] = None,
        fixed_split_size: Optional[int] = None,
        disable_split_kv: bool = False,
        bf16_pv_exact_range: bool = False,
    ) -> None:
        r"""Plan for ragged queries ``qo_indptr`` and ragged keys/values ``kv_indptr`` (both int32
        ``[batch_size + 1]``).  Options as :meth:`BatchPrefillWithPagedKVCacheWrapper.plan`."""
        self._bf16_pv_mode = 1 if bf16_pv_exact_range else 0
        self._prefix_len_ptr, self._token_pos_in_items_ptr, self._max_item_len_ptr, self._token_pos_in_items_len = \
            _check_multi_item_args(prefix_len_ptr, token_pos_in_items_ptr, max_item_len_ptr, token_pos_in_items_len,
                                   len(qo_indptr) - 1, self.device)
        _check_pos_encoding_mode(pos_encoding_mode)
        q_data_type, kv_data_type = canonicalize_qkv_dtypes(q_data_type, kv_data_type)
        if logits_soft_cap is None:
            logits_soft_cap = 0.0
        if head_dim_vo is None:
            head_dim_vo = head_dim_qk
        self._qkvo = head_dim_vo != head_dim_qk
        if self._qkvo:
            _check_qkvo_config(head_dim_qk, head_dim_vo, q_data_type, kv_data_type, pos_encoding_mode,
                               logits_soft_cap, custom_mask is not None or packed_custom_mask is not None
                               or prefix_len_ptr is not None)
        self._head_dim_vo = head_dim_vo
        batch_size = len(qo_indptr) - 1
        if len(kv_indptr) != batch_size + 1:
            raise ValueError("The kv_indptr length should be equal to qo_indptr length.")
        qo_indptr_host = qo_indptr.to("cpu").contiguous()
        kv_indptr_host = kv_indptr.to("cpu").contiguous()
        kv_len_arr = (kv_indptr_host[1:] - kv_indptr_host[:-1]).to(torch.int32).contiguous()
        _check_multi_item_rows(self._prefix_len_ptr, self._token_pos_in_items_len, kv_len_arr)
        total_num_rows = int(qo_indptr_host[-1])
        self._custom_mask_buf, self._mask_indptr_buf = _plan_custom_mask(
            self, custom_mask, packed_custom_mask, qo_indptr_host, kv_len_arr, non_blocking)
        if self._custom_mask_buf is not None:
            causal = False
        self._bind_index_tensors(batch_size, non_blocking, qo_indptr=qo_indptr, kv_indptr=kv_indptr)
        self._plan_info = _lib.batch_prefill_plan(
            self._float_workspace_buffer, self._int_workspace_buffer, self._pin_memory_int_workspace_buffer,
            qo_indptr_host, kv_indptr_host, kv_len_arr, total_num_rows, batch_size, num_qo_heads, num_kv_heads, 1,
            self._use_cuda_graph, head_dim_qk, head_dim_vo, causal, window_left,
            -1 if fixed_split_size is None else fixed_split_size, disable_split_kv,
            "BatchPrefillWithRaggedKVCacheWrapper.plan")
        self._batch_size = batch_size
        self._num_qo_heads = num_qo_heads
        self._num_kv_heads = num_kv_heads
        self._head_dim = head_dim_qk
        self._total_num_rows = total_num_rows
        self._total_kv_rows = int(kv_indptr_host[-1])
        self._cached_q_data_type = q_data_type
        self._cached_kv_data_type = kv_data_type
        self._causal = causal
        self._set_run_options(pos_encoding_mode, window_left, logits_soft_cap, sm_scale, rope_scale, rope_theta)

    begin_forward = plan

    def run(
        self,
        q: torch.Tensor,
        k: torch.Tensor,
        v: torch.Tensor,
        *args,
        q_scale: Optional[float] = None,
        k_scale: Optional[float] = None,
        v_scale: Optional[float] = None,
        out: Optional[torch.Tensor] = None,
        lse: Optional[torch.Tensor] = None,
        return_lse: bool = False,
        enable_pdl: Optional[bool] = None,
    ) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        r"""q ``[qo_indptr[-1], num_qo_heads, head_dim]``; k, v ragged as described in the class docstring.

        A wrapper built with the reference's "AttentionSink" ``jit_args`` (tests/attention/test_attention_sink.py
        :162-235) is called as ``run(q, k, v, sink, sm_scale)``: ``sink`` is float32 ``[num_qo_heads]``, one logit per
        head that joins the softmax denominator (see :meth:`BatchPrefillWithPagedKVCacheWrapper.run`); the returned
        state must not be merged again.  Not at head_dim_qk 192 / head_dim_vo 128."""
        args, sinks, sm_scale = self._sink_variant_args(args, None)
        self._check_run_args(args)
        for t, name in ((q, "q"), (k, "k"), (v, "v")):
            _lib.require_gpu_tensor(t, name)
        _check_cached_qkv_data_type(q, k, self._cached_q_data_type, self._cached_kv_data_type)
        if is_float8(q):
            raise ValueError("fp8 queries are supported by the paged wrapper only")
        if self._qkvo:
            if sinks is not None:
                raise ValueError("attention sinks are not supported at head_dim_qk 192 / head_dim_vo 128")
            return self._run_qkvo(q, k, v, q_scale, k_scale, v_scale, out, lse, return_lse)
        if k.shape != v.shape or k.stride() != v.stride() or k.dim() != 3 or k.stride(-1) != 1:
            raise ValueError("k and v must be 3-D with equal shapes/strides, contiguous in head_dim")
        kv = ragged_kv(k, v, self._kv_layout, self._kv_indptr_buf, self._batch_size)
        nnz_kv = dense_kv_dims(k, self._kv_layout)[0]
        if kv.num_kv_heads != self._num_kv_heads or kv.head_dim != self._head_dim or nnz_kv < self._total_kv_rows:
            raise ValueError("k/v shape does not match the plan")
        if q.dim() != 3 or q.shape[0] != self._total_num_rows or q.shape[1] != self._num_qo_heads:
            raise ValueError("q shape does not match the plan")
        return _run_batch_prefill(self, "BatchPrefillWithRaggedKVCacheWrapper.run", q, kv, q.dtype, out, lse,
                                  return_lse, self._window_left, q_scale, k_scale, v_scale, sinks=sinks,
                                  sm_scale=sm_scale)

    def _run_qkvo(self, q, k, v, q_scale, k_scale, v_scale, out, lse, return_lse):
        """run() of a head_dim_qk 192 / head_dim_vo 128 plan: k and v by their own strides, no copy."""
        _check_qkvo_kv(k, v)
        (nnz_k, hk, _, _), dk = dense_kv_dims(k, self._kv_layout), k.shape[2]
        (nnz_v, hv, _, _), dv = dense_kv_dims(v, self._kv_layout), v.shape[2]
        if (hk, dk) != (self._num_kv_heads, self._head_dim) or (hv, dv) != (self._num_kv_heads, self._head_dim_vo):
            raise ValueError(f"k must be [.., {self._num_kv_heads}, {self._head_dim}] and v [.., {self._num_kv_heads}, "
                             f"{self._head_dim_vo}] as planned, got {tuple(k.shape)} / {tuple(v.shape)}")
        if min(nnz_k, nnz_v) < self._total_kv_rows or v.dtype != k.dtype:
            raise ValueError("k / v hold fewer rows than kv_indptr[-1], or differ in dtype")
        if q.dim() != 3 or q.shape != (self._total_num_rows, self._num_qo_heads, self._head_dim):
            raise ValueError("q shape does not match the plan")
        if q.stride(-1) != 1:
            q = q.contiguous()
        out, lse = _out_and_lse(q, out, lse, return_lse, (q.shape[0], q.shape[1], self._head_dim_vo), q.dtype)
        sm_scale = _resolve_logits_params(self._head_dim, self._sm_scale, q_scale, k_scale, None, None,
                                          None)["sm_scale"]
        params = _qkvo_params(q, k, v, self._kv_layout, out, lse, self._causal,
                              self._window_left, sm_scale, self._bf16_pv_mode,
                              qo_indptr=self._qo_indptr_buf.data_ptr(), kv_indptr=self._kv_indptr_buf.data_ptr(),
                              batch_size=self._batch_size)
        with torch.cuda.device(q.device):
            _lib.check(
                _lib.lib().fi_batch_prefill_qkvo_run(
                    *self._workspace_args, self._plan_info, _lib.FI_PREFILL_PLAN_INFO_LEN, C.byref(params),
                    _lib.current_stream(q.device),
                ),
                "BatchPrefillWithRaggedKVCacheWrapper.run",
            )
        if v_scale is not None:
            out = _apply_v_scale(out, v_scale)
        return (out, lse) if return_lse else out

    run_return_lse = functools.partialmethod(run, return_lse=True)

    def end_forward(self) -> None:
        pass


def trtllm_batch_context_with_kv_cache(
    query: torch.Tensor,
    kv_cache: Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]],
    workspace_buffer: torch.Tensor,
    block_tables: torch.Tensor,
    seq_lens: torch.Tensor,
    max_q_len: int,
    max_kv_len: int,
    bmm1_scale: float,
    bmm2_scale: float,
    batch_size: int,
    cum_seq_lens_q: torch.Tensor,
    cum_seq_lens_kv: torch.Tensor,
    window_left: int = -1,
    out: Optional[torch.Tensor] = None,
    out_dtype: Optional[Union[torch.dtype, str]] = None,
    o_sf_scale: Optional[float] = None,
    o_sf_vec_size: Optional[int] = None,
    enable_pdl: Optional[bool] = None,
    sinks: Optional[List[torch.Tensor]] = None,
) -> torch.Tensor:
    r"""Plan-free causal prefill / chunked prefill / mixed step over a paged KV cache (ref: flashinfer/prefill.py
    :3314-3334): a dense block table, device-resident kv lengths and query offsets instead of ``plan()``.  The work list,
    the page table and the query offsets the kernels read are written by kernels on the current stream
    (fi_batch_prefill_plan_device), then the kernels of :class:`BatchPrefillWithPagedKVCacheWrapper` run on them: two
    planner launches, the prefill launch, and the merge when the plan splits the kv axis.  There is no host
    synchronisation and nothing is allocated by a length, so the whole call can be captured in a graph; a replay plans
    again from what ``block_tables``, ``seq_lens`` and ``cum_seq_lens_q`` hold then.

    query : ``[num_tokens, num_qo_heads, head_dim]``, float16 or bfloat16 (rows may be strided), or float8_e4m3fn with
        an e4m3 cache; then ``out`` or ``out_dtype`` must name float16 or bfloat16.
    kv_cache : one tensor ``[num_pages, 2, num_kv_heads, page_size, head_dim]`` (the HND layout), or a ``(k, v)`` tuple
        of ``[num_pages, num_kv_heads, page_size, head_dim]`` tensors; the query's dtype, or fp8 under a 16-bit query.
    workspace_buffer : one buffer on the query's device; the work list, the page table and the f32 partial states are
        carved out of it.  It need not be zeroed.  ValueError names the bytes needed when it is too small.
    block_tables : int32 ``[batch_size, max_blocks]``; row ``b`` lists the pages of request ``b``.
    seq_lens : int32 (or uint32) ``[batch_size]`` on the device: kv tokens per request, the new ones included.  A
        length beyond ``max_blocks * page_size`` is CLAMPED to it, a negative one to 0 (the host never sees the values).
    max_q_len : unused.  max_kv_len : checked against ``max_blocks * page_size``; otherwise unused.
    bmm1_scale : the full scale of the logits (``sm_scale``).  bmm2_scale : multiplies the output.
    batch_size : must equal ``block_tables.shape[0]``.
    cum_seq_lens_q : int32 ``[batch_size + 1]`` on the device: request ``b`` owns the query rows
        ``cum_seq_lens_q[b]:cum_seq_lens_q[b + 1]``, which sit at the END of its ``seq_lens[b]`` kv tokens (causal).
        The kernels read a copy clamped to ``[0, num_tokens]`` and made non-decreasing.  Rows of ``out`` from
        ``cum_seq_lens_q[batch_size]`` on are left untouched.
    cum_seq_lens_kv : accepted and not read.
    window_left : sliding window, ``-1`` for none.
    out : optional output ``[num_tokens, num_qo_heads, head_dim]``.  out_dtype : its dtype (a 16-bit query's own).
    sinks : optional float32 ``[num_qo_heads]`` attention-sink logits (or a one-element list holding them); float16 /
        bfloat16 queries only.
    enable_pdl : accepted and ignored.

    Not offered (NotImplementedError): ``out_dtype="nvfp4"`` / an FP4Tensor ``out`` / ``o_sf_scale`` /
    ``o_sf_vec_size``, an fp8 output, the ``[num_pages, 1, ...]`` cache with K and V shared, and an e5m2 query.
    """
    name = "trtllm_batch_context_with_kv_cache"
    if query.dtype == torch.float8_e5m2:
        raise NotImplementedError(f"{name}: an e5m2 query is not supported (float16 / bfloat16 / float8_e4m3fn)")
    _refuse_fp4_out_and_shared_kv(name, kv_cache, out, out_dtype, o_sf_scale, o_sf_vec_size)
    o_dtype = out.dtype if out is not None else None if out_dtype is None else canonicalize_torch_dtype(out_dtype)
    if o_dtype in (torch.float8_e4m3fn, torch.float8_e5m2):
        raise NotImplementedError(f"{name}: an fp8 output is not supported (float16 / bfloat16)")
    for arg, t in (("query", query), ("workspace_buffer", workspace_buffer), ("block_tables", block_tables),
                   ("seq_lens", seq_lens), ("cum_seq_lens_q", cum_seq_lens_q)):
        _lib.require_gpu_tensor(t, arg)
    k_cache, v_cache = _hnd_cache_views(kv_cache)
    fp8_query = query.dtype == torch.float8_e4m3fn
    if query.dtype not in (torch.float16, torch.bfloat16, torch.float8_e4m3fn) or query.dim() != 3 \
            or query.stride(-1) != 1:
        raise ValueError("query must be a float16 / bfloat16 / float8_e4m3fn [num_tokens, num_qo_heads, head_dim] "
                         "tensor, contiguous in head_dim")
    num_tokens, num_qo_heads, head_dim = query.shape
    if batch_size != block_tables.shape[0]:
        raise ValueError(f"batch_size {batch_size} differs from block_tables.shape[0] = {block_tables.shape[0]}")
    seq_lens = _check_block_tables_and_lens(block_tables, seq_lens, workspace_buffer, batch_size)
    if cum_seq_lens_q.dtype != torch.int32 or cum_seq_lens_q.shape != (batch_size + 1,) \
            or not cum_seq_lens_q.is_contiguous():
        raise ValueError(f"cum_seq_lens_q must be a contiguous int32 tensor of shape [{batch_size + 1}]")
    if fp8_query:
        if o_dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("an fp8 query needs out or out_dtype to name float16 or bfloat16")
        if k_cache.dtype != torch.float8_e4m3fn:
            raise ValueError(f"an fp8 e4m3 query needs an e4m3 kv_cache, got {k_cache.dtype}")
    elif o_dtype is None:
        o_dtype = query.dtype
    elif o_dtype != query.dtype:
        raise ValueError(f"the output dtype {o_dtype} differs from the query's {query.dtype}")
    if out_dtype is not None and canonicalize_torch_dtype(out_dtype) != o_dtype:
        raise ValueError(f"out_dtype {out_dtype} differs from out's {o_dtype}")
    out = _out_or_empty(out, query.shape, o_dtype, query.device)
    sinks = _one_sinks_tensor(sinks, num_qo_heads, query.device)
    if sinks is not None and fp8_query:
        raise ValueError("sinks need a float16 / bfloat16 query")

    max_blocks = block_tables.shape[1]
    # the cache view; its three page-table pointers are set below, once the planner has said where it writes them
    kv, page_size, num_kv_heads, kv_head_dim = paged_kv(k_cache, v_cache, "HND", block_tables, None, None, batch_size)
    if kv_head_dim != head_dim:
        raise ValueError(f"head_dim of query ({head_dim}) and kv_cache ({kv_head_dim}) differ")
    _check_len_fits_block_tables("max_kv_len", max_kv_len, max_blocks, page_size)
    if batch_size == 0 or num_tokens == 0:
        return out

    plan = _lib.fi_batch_prefill_plan_device_params_t(
        block_tables=block_tables.data_ptr(), seq_lens=seq_lens.data_ptr(), cum_seq_lens_q=cum_seq_lens_q.data_ptr(),
        block_tables_stride=block_tables.stride(0), batch_size=batch_size, max_blocks=max_blocks, page_size=page_size,
        total_num_rows=num_tokens, num_qo_heads=num_qo_heads, num_kv_heads=num_kv_heads, head_dim=head_dim,
        q_dtype=_lib.fi_dtype(query.dtype), kv_dtype=_lib.fi_dtype(k_cache.dtype), window_left=window_left,
        max_items_hint=0)
    _device_plan_regions(workspace_buffer, plan, "fi_batch_prefill_plan_device_workspace", name)
    plan_info = (C.c_int64 * _lib.FI_PREFILL_PLAN_INFO_LEN)()
    csr = (C.c_int64 * 4)()
    # bmm2_scale rides on the kernels' per-kv-head V scale, so rows no request owns stay untouched
    scale_v = None if bmm2_scale == 1.0 else torch.full((num_kv_heads,), float(bmm2_scale), dtype=torch.float32,
                                                        device=query.device)
    params = _lib.fi_batch_prefill_params_t(
        q=query.data_ptr(), q_stride_n=query.stride(0), q_stride_h=query.stride(1), kv=kv, o=out.data_ptr(),
        scale_v=_lib.ptr(scale_v), num_qo_heads=num_qo_heads, q_dtype=plan.q_dtype, o_dtype=_lib.fi_dtype(o_dtype),
        mask_mode=MaskMode.CAUSAL.value, pos_encoding_mode=PosEncodingMode.NONE.value, window_left=window_left,
        **_resolve_logits_params(head_dim, bmm1_scale, None, None, None, None, None))
    lib = _lib.lib()
    with torch.cuda.device(query.device):
        stream = _lib.current_stream(query.device)
        _lib.check(lib.fi_batch_prefill_plan_device(C.byref(plan), plan_info, csr, stream), name)
        # the page table and the clamped query offsets the planner's kernels write, in place of what plan() is given
        params.kv.indptr, params.kv.indices, params.kv.last_page_len, params.qo_indptr = (
            plan.int_ws + off for off in csr)
        _lib.check(lib.fi_batch_prefill_paged_run_sinks(plan.float_ws, plan.float_ws_bytes, plan.int_ws,
                                                        plan.int_ws_bytes, plan_info, _lib.FI_PREFILL_PLAN_INFO_LEN,
                                                        C.byref(params), _lib.ptr(sinks), stream), name)
    return out
