"""Decode attention operators: ``single_decode_with_kv_cache``,
``BatchDecodeWithPagedKVCacheWrapper`` (plan / run split) and the plan-free
``trtllm_batch_decode_with_kv_cache`` and ``trtllm_batch_decode_with_kv_cache_mla`` (the work list is planned on the
device).

Same names, arguments, defaults and error behaviour as the reference's ``flashinfer/decode.py``
(single :389-578; wrapper :581-1410; CUDA-graph wrapper :1413-1480; plan-free :2054-2071, MLA :2298-2315), with the JIT
module layer replaced by the ahead-of-time C ABI of libfi_mi355.so.  The kernels are csrc/decode_kernel.h and, for MLA,
csrc/mla.hip.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Any, List, Optional, Tuple, Union

import torch

from . import _lib
from ._plan_free import (_check_block_tables_and_lens, _check_len_fits_block_tables, _device_plan_regions,
                         _hnd_cache_views, _one_sinks_tensor, _out_or_empty, _refuse_fp4_out_and_shared_kv)
from ._wrapper import BatchAttentionWrapper
from .page import get_seq_lens
from .utils import (
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
    paged_kv,
)


def fast_decode_plan(
    self: "BatchDecodeWithPagedKVCacheWrapper",
    indptr: torch.Tensor,
    indices: torch.Tensor,
    last_page_len: torch.Tensor,
    num_qo_heads: int,
    num_kv_heads: int,
    head_dim: int,
    page_size: int,
    pos_encoding_mode: str = "NONE",
    window_left: int = -1,
    logits_soft_cap: Optional[float] = None,
    q_data_type: Optional[Union[str, torch.dtype]] = None,
    kv_data_type: Optional[Union[str, torch.dtype]] = None,
    data_type: Optional[Union[str, torch.dtype]] = None,
    sm_scale: Optional[float] = None,
    rope_scale: Optional[float] = None,
    rope_theta: Optional[float] = None,
    non_blocking: bool = True,
    fixed_split_size: Optional[int] = None,
    disable_split_kv: bool = False,
    global_override_indptr_cpu: Optional[torch.Tensor] = None,
) -> None:
    """A faster :meth:`BatchDecodeWithPagedKVCacheWrapper.plan` for multi-step draft decoding
    (ref: flashinfer/decode.py:2416-2579): the device-to-device copies into the graph buffers are skipped
    (the caller wrote them in place; outside graph mode the given tensors are adopted without a copy), and
    ``global_override_indptr_cpu`` supplies the host page-table prefix sums so that no device-to-host copy
    is needed.  Bind it with ``wrapper.begin_forward = functools.partial(fast_decode_plan, wrapper)``."""
    if data_type is None and q_data_type is None:
        q_data_type = "float16"
    self.plan(
        indptr, indices, last_page_len, num_qo_heads, num_kv_heads, head_dim, page_size,
        pos_encoding_mode=pos_encoding_mode, window_left=window_left, logits_soft_cap=logits_soft_cap,
        q_data_type=q_data_type, kv_data_type=kv_data_type, data_type=data_type, sm_scale=sm_scale,
        rope_scale=rope_scale, rope_theta=rope_theta, non_blocking=non_blocking,
        fixed_split_size=None,  # as the reference: not forwarded by the fast path
        disable_split_kv=disable_split_kv, _fast=True, _indptr_host=global_override_indptr_cpu,
    )


def single_decode_with_kv_cache(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    kv_layout: str = "NHD",
    pos_encoding_mode: str = "NONE",
    use_tensor_cores: bool = False,
    q_scale: Optional[float] = None,
    k_scale: Optional[float] = None,
    v_scale: Optional[float] = None,
    window_left: int = -1,
    logits_soft_cap: Optional[float] = None,
    sm_scale: Optional[float] = None,
    rope_scale: Optional[float] = None,
    rope_theta: Optional[float] = None,
    return_lse: bool = False,
) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    r"""Decode attention with KV cache for a single request.

    Parameters
    ----------
    q : torch.Tensor
        The query tensor, shape: ``[num_qo_heads, head_dim]``.
    k, v : torch.Tensor
        ``[kv_len, num_kv_heads, head_dim]`` if :attr:`kv_layout` is ``NHD``, or
        ``[num_kv_heads, kv_len, head_dim]`` if ``HND``.
    kv_layout : str
        ``NHD`` or ``HND``.
    pos_encoding_mode : str
        ``NONE`` / ``ROPE_LLAMA`` (rotary embedding applied inside the kernel) / ``ALIBI``.
    use_tensor_cores : bool
        Use the MFMA (prefill-kernel) path; numerically equivalent.
    q_scale, k_scale, v_scale : Optional[float]
        Calibration scales for fp8 inputs (folded into ``sm_scale`` / applied to the output).
    window_left : int
        Left (inclusive) attention window; ``-1`` = whole sequence.
    logits_soft_cap : Optional[float]
        If > 0, logits are capped as ``cap * tanh(x / cap)``.
    sm_scale : Optional[float]
        Softmax scale, default ``1 / sqrt(head_dim)``.
    rope_scale, rope_theta : Optional[float]
        RoPE interpolation scale (default 1) and theta (default 1e4).
    return_lse : bool
        Also return the base-2 log-sum-exp of the attention logits, shape ``[num_qo_heads]``.
    """
    _check_pos_encoding_mode(pos_encoding_mode)
    _check_kv_layout(kv_layout)
    _lib.require_gpu_tensor(q, "q")
    _lib.require_gpu_tensor(k, "k")
    _lib.require_gpu_tensor(v, "v")
    if q.dim() != 2 or k.dim() != 3 or v.shape != k.shape:
        raise ValueError("q must be [num_qo_heads, head_dim]; k and v must be 3-D with equal shapes")
    head_dim = q.shape[-1]
    num_qo_heads = q.shape[0]
    kv_len, num_kv_heads, stride_n, stride_h = dense_kv_dims(k, kv_layout)
    if k.stride() != v.stride() or k.stride(-1) != 1 or q.stride(-1) != 1:
        raise ValueError("k and v must share strides and q/k/v must be contiguous in head_dim")
    if num_qo_heads % num_kv_heads != 0:
        raise ValueError("num_qo_heads must be a multiple of num_kv_heads")

    tmp = _get_cache_buf("single_decode_with_kv_cache_tmp", 32 * 1024 * 1024, q.device)
    out = torch.empty_like(q)
    lse = None
    if return_lse:
        lse = torch.empty((num_qo_heads,), dtype=torch.float32, device=q.device)
    alibi = None
    if pos_encoding_mode == "ALIBI":
        alibi = _get_cache_alibi_slopes_buf(num_qo_heads, q.device)

    params = _lib.fi_single_decode_params_t(
        q=q.data_ptr(), q_stride_h=q.stride(0), k=k.data_ptr(), v=v.data_ptr(),
        kv_stride_n=stride_n, kv_stride_h=stride_h, o=out.data_ptr(), lse=_lib.ptr(lse),
        alibi_slopes=_lib.ptr(alibi), kv_len=kv_len, num_qo_heads=num_qo_heads,
        num_kv_heads=num_kv_heads, head_dim=head_dim, q_dtype=_lib.fi_dtype(q.dtype),
        kv_dtype=_lib.fi_dtype(k.dtype), pos_encoding_mode=PosEncodingMode[pos_encoding_mode].value,
        window_left=window_left,
        **_resolve_logits_params(head_dim, sm_scale, q_scale, k_scale, logits_soft_cap, rope_scale, rope_theta),
    )
    with torch.cuda.device(q.device):
        _lib.check(
            _lib.lib().fi_single_decode_run(
                C.byref(params), tmp.data_ptr(), _lib.nbytes(tmp), _lib.current_stream(q.device)
            ),
            "single_decode_with_kv_cache",
        )
    if v_scale is not None:
        out = _apply_v_scale(out, v_scale)
    return (out, lse) if return_lse else out


class BatchDecodeWithPagedKVCacheWrapper(BatchAttentionWrapper):
    r"""Decode attention over a paged KV cache for a batch of requests.

    ``plan()`` is host work done once per batch shape and reused by every layer; ``run()`` launches the
    kernels on the current stream.  See the reference docstring (flashinfer/decode.py:581-646) for the
    page-table layout; the example there runs unchanged:

    >>> workspace_buffer = torch.zeros(128 * 1024 * 1024, dtype=torch.uint8, device="cuda:0")
    >>> decode_wrapper = flashinfer.BatchDecodeWithPagedKVCacheWrapper(workspace_buffer, "NHD")
    >>> decode_wrapper.plan(kv_page_indptr, kv_page_indices, kv_last_page_len, num_qo_heads,
    ...                     num_kv_heads, head_dim, page_size, pos_encoding_mode="NONE",
    ...                     data_type=torch.float16)
    >>> o = decode_wrapper.run(q, kv_cache)
    """

    def __init__(
        self,
        float_workspace_buffer: torch.Tensor,
        kv_layout: str = "NHD",
        use_cuda_graph: bool = False,
        use_tensor_cores: bool = False,
        paged_kv_indptr_buffer: Optional[torch.Tensor] = None,
        paged_kv_indices_buffer: Optional[torch.Tensor] = None,
        paged_kv_last_page_len_buffer: Optional[torch.Tensor] = None,
        backend: str = "auto",
        jit_args: Optional[List[Any]] = None,
    ) -> None:
        r"""Parameters as the reference (flashinfer/decode.py:647-776).

        float_workspace_buffer : split-KV partial states live here (128 MB recommended).
        use_cuda_graph : keep the launch shape fixed so ``run`` can be captured in a hipGraph;
            the three ``paged_kv_*_buffer`` tensors are then required and the batch size is fixed.
        use_tensor_cores : accepted; selects the MFMA path when available.
        backend : ``auto`` / ``fa2`` (one native backend exists; NVIDIA-only names are rejected).
        jit_args : must be None -- there is no JIT in this build (attention sinks go through ``run(sinks=)``).
        """
        _check_kv_layout(kv_layout)
        super().__init__(float_workspace_buffer, use_cuda_graph, backend, ("auto", "fa2"), jit_args)
        self._kv_layout = kv_layout
        if use_cuda_graph:
            if not torch.is_tensor(paged_kv_indptr_buffer):
                raise ValueError("paged_kv_indptr_buffer should be a torch.Tensor in cudagraph mode")
            if not torch.is_tensor(paged_kv_indices_buffer):
                raise ValueError("paged_kv_indices_buffer should be a torch.Tensor in cudagraph mode")
            if not torch.is_tensor(paged_kv_last_page_len_buffer):
                raise ValueError(
                    "paged_kv_last_page_len_buffer should be a torch.Tensor in cudagraph mode"
                )
            self._fixed_batch_size = len(paged_kv_last_page_len_buffer)
            if len(paged_kv_indptr_buffer) != self._fixed_batch_size + 1:
                raise ValueError("The size of paged_kv_indptr_buffer should be batch_size + 1")
        self._paged_kv_indptr_buf = paged_kv_indptr_buffer
        self._paged_kv_indices_buf = paged_kv_indices_buffer
        self._paged_kv_last_page_len_buf = paged_kv_last_page_len_buffer
        self._use_tensor_cores = use_tensor_cores
        self._run_cache = None
        self._plan_serial = 0

    @property
    def use_tensor_cores(self) -> bool:
        return self._use_tensor_cores

    def reset_workspace_buffer(
        self, float_workspace_buffer: torch.Tensor, int_workspace_buffer: torch.Tensor
    ) -> None:
        r"""Swap the workspaces; a new pinned mirror of the int workspace is allocated."""
        self._run_cache = None  # it holds the old workspaces' pointers
        super().reset_workspace_buffer(float_workspace_buffer, int_workspace_buffer)

    def plan(
        self,
        indptr: torch.Tensor,
        indices: torch.Tensor,
        last_page_len: torch.Tensor,
        num_qo_heads: int,
        num_kv_heads: int,
        head_dim: int,
        page_size: int,
        pos_encoding_mode: str = "NONE",
        window_left: int = -1,
        logits_soft_cap: Optional[float] = None,
        q_data_type: Optional[Union[str, torch.dtype]] = "float16",
        kv_data_type: Optional[Union[str, torch.dtype]] = None,
        data_type: Optional[Union[str, torch.dtype]] = None,
        sm_scale: Optional[float] = None,
        rope_scale: Optional[float] = None,
        rope_theta: Optional[float] = None,
        non_blocking: bool = True,
        block_tables: Optional[torch.Tensor] = None,
        seq_lens: Optional[torch.Tensor] = None,
        fixed_split_size: Optional[int] = None,
        disable_split_kv: bool = False,
        _fast: bool = False,
        _indptr_host: Optional[torch.Tensor] = None,
    ) -> None:
        r"""Plan batch decode for the given page table (ref: flashinfer/decode.py:810-1104).

        indptr : ``[batch_size + 1]`` int32, indices : ``[indptr[-1]]`` int32,
        last_page_len : ``[batch_size]`` int32 (1 <= last_page_len <= page_size).
        The remaining arguments configure the attention variant exactly as in the reference.
        ``plan`` is synchronous host code and must not be captured in a graph.
        """
        _check_pos_encoding_mode(pos_encoding_mode)
        batch_size = len(last_page_len)
        if logits_soft_cap is None:
            logits_soft_cap = 0.0
        # fast_decode_plan: the caller wrote the graph buffers in place; without a graph its tensors are adopted
        self._bind_index_tensors(batch_size, non_blocking, prefix=("paged_kv_indices",), adopt=_fast,
                                 paged_kv_indptr=indptr, paged_kv_indices=indices,
                                 paged_kv_last_page_len=last_page_len)
        indptr_host = (indptr if _indptr_host is None else _indptr_host).to("cpu").contiguous()
        if indptr_host.dtype != torch.int32 or len(indptr_host) != batch_size + 1:
            raise ValueError("indptr must be int32 with batch_size + 1 entries")

        if data_type is not None:
            if q_data_type is None:
                q_data_type = data_type
            if kv_data_type is None:
                kv_data_type = data_type
        q_data_type, kv_data_type = canonicalize_qkv_dtypes(q_data_type, kv_data_type)
        if fixed_split_size is not None and not self.use_tensor_cores:
            raise ValueError("fixed_split_size is only supported by tensor core decode for now.")

        self._cached_q_data_type = q_data_type
        self._cached_kv_data_type = kv_data_type
        self._batch_size = batch_size
        self._num_qo_heads = num_qo_heads
        self._num_kv_heads = num_kv_heads
        self._head_dim = head_dim
        self._page_size = page_size
        if _fast:
            self._kv_lens_host = None  # not needed by run(); skipping it saves a device-to-host copy
        elif seq_lens is None:
            last_page_len_host = last_page_len.to("cpu")
            self._kv_lens_host = get_seq_lens(indptr_host, last_page_len_host, page_size)
        else:
            self._kv_lens_host = seq_lens.cpu()

        # max_grid_hint 1: batch * heads >= 1 always, so the planner never splits
        self._plan_info = _lib.batch_decode_plan(
            self._float_workspace_buffer, self._int_workspace_buffer, self._pin_memory_int_workspace_buffer,
            indptr_host, batch_size, num_qo_heads, num_kv_heads, page_size, self._use_cuda_graph, head_dim,
            q_data_type, kv_data_type, 1 if disable_split_kv else 0, window_left,
            "BatchDecodeWithPagedKVCacheWrapper.plan")
        self._plan_serial += 1
        self._run_cache = None
        self._set_run_options(pos_encoding_mode, window_left, logits_soft_cap, sm_scale, rope_scale, rope_theta)

    begin_forward = plan

    def forward(
        self,
        q: torch.Tensor,
        paged_kv_cache: Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]],
        pos_encoding_mode: str = "NONE",
        q_scale: Optional[float] = None,
        k_scale: Optional[float] = None,
        v_scale: Optional[float] = None,
        window_left: int = -1,
        logits_soft_cap: Optional[float] = None,
        sm_scale: Optional[float] = None,
        rope_scale: Optional[float] = None,
        rope_theta: Optional[float] = None,
    ) -> torch.Tensor:
        r"""Warning: this function is deprecated, please use :meth:`run` instead."""
        self._set_run_options(pos_encoding_mode, window_left, logits_soft_cap, sm_scale, rope_scale, rope_theta)
        self._run_cache = None
        return self.run(q, paged_kv_cache, q_scale=q_scale, k_scale=k_scale, v_scale=v_scale)

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
        q_len_per_req: Optional[int] = 1,
    ) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        r"""Compute batch decode attention between ``q`` and the paged KV cache.

        q : ``[batch_size, num_qo_heads, head_dim]``.
        paged_kv_cache : a 5-D tensor ``[max_num_pages, 2, page_size, num_kv_heads, head_dim]`` (NHD) /
            ``[max_num_pages, 2, num_kv_heads, page_size, head_dim]`` (HND), or a ``(k_cache, v_cache)``
            tuple of 4-D tensors.
        sinks : optional float32 ``[num_qo_heads]`` on the wrapper's device, contiguous: one attention-sink logit per
            head (natural-log units, not multiplied by ``sm_scale``) that joins the softmax denominator without a
            value vector (ref: flashinfer/jit/attention/variants.py:17-53).  ``-inf`` switches a head's sink off.  The
            returned logsumexp includes the sink, so a state with a folded sink must not be merged again
            (``merge_state`` and the cascade wrappers would count it twice).  The tensor is read when the kernels
            run: a captured ``run`` sees the values it holds at replay.
        Returns the output ``[batch_size, num_qo_heads, head_dim]`` (and the base-2 logsumexp
        ``[batch_size, num_qo_heads]`` when ``return_lse``).  (ref: flashinfer/decode.py:1163-1374)
        """
        if self._plan_info is None:
            raise RuntimeError("plan() must be called before run()")
        sinks_ptr = 0 if sinks is None else self._sinks_ptr(sinks, q)
        if args:
            raise ValueError("additional kernel arguments require jit_args, which is not supported")
        window_left = self._window_left if window_left is None else window_left
        # window_left is part of the plan in the reference; keep the same contract
        assert window_left == self._window_left
        if return_lse and lse is None:
            lse = torch.empty((q.size(0), q.size(1)), dtype=torch.float32, device=q.device)
        if out is None:
            out = torch.empty(q.shape, dtype=q.dtype, device=q.device)

        # Steady-state calls (same tensors every layer / step) reuse the validated argument block.
        cache_t = paged_kv_cache if torch.is_tensor(paged_kv_cache) else paged_kv_cache[0]
        key = (q.data_ptr(), q.stride(), q.shape, cache_t.data_ptr(), cache_t.stride(), cache_t.shape,
               None if torch.is_tensor(paged_kv_cache) else paged_kv_cache[1].data_ptr(),
               out.data_ptr(), lse.data_ptr() if return_lse else 0, q_scale, k_scale, self._plan_serial, sinks_ptr)
        cached = self._run_cache
        if cached is not None and cached[0] == key:
            params = cached[1]
        else:
            params = self._build_run_params(q, paged_kv_cache, q_scale, k_scale, out, lse if return_lse else None)
            self._run_cache = (key, params, q, paged_kv_cache)  # keep the tensors alive with the pointers
        dev_index = q.device.index
        if sinks_ptr:
            if torch.cuda.current_device() == dev_index:
                status = self._lib_run_sinks(self._fws_ptr, self._fws_bytes, self._iws_ptr, self._iws_bytes,
                                             self._plan_info, _lib.FI_DECODE_PLAN_INFO_LEN, params, sinks_ptr,
                                             torch.cuda.current_stream().cuda_stream)
            else:
                with torch.cuda.device(q.device):
                    status = self._lib_run_sinks(self._fws_ptr, self._fws_bytes, self._iws_ptr, self._iws_bytes,
                                                 self._plan_info, _lib.FI_DECODE_PLAN_INFO_LEN, params, sinks_ptr,
                                                 torch.cuda.current_stream().cuda_stream)
        elif torch.cuda.current_device() == dev_index:
            status = self._lib_run(self._fws_ptr, self._fws_bytes, self._iws_ptr, self._iws_bytes,
                                   self._plan_info, _lib.FI_DECODE_PLAN_INFO_LEN, params,
                                   torch.cuda.current_stream().cuda_stream)
        else:
            with torch.cuda.device(q.device):
                status = self._lib_run(self._fws_ptr, self._fws_bytes, self._iws_ptr, self._iws_bytes,
                                       self._plan_info, _lib.FI_DECODE_PLAN_INFO_LEN, params,
                                       torch.cuda.current_stream().cuda_stream)
        if status != 0:
            _lib.check(status, "BatchDecodeWithPagedKVCacheWrapper.run")
        if v_scale is not None:
            out = _apply_v_scale(out, v_scale)
        return (out, lse) if return_lse else out

    def _build_run_params(self, q, paged_kv_cache, q_scale, k_scale, out, lse):
        """Validate the run() arguments against the plan and build the C argument block."""
        _lib.require_gpu_tensor(q, "q")
        k_cache, v_cache = _unpack_paged_kv_cache(paged_kv_cache, self._kv_layout)
        _check_cached_qkv_data_type(q, k_cache, self._cached_q_data_type, self._cached_kv_data_type)
        kv, page_size, num_kv_heads, head_dim = paged_kv(
            k_cache, v_cache, self._kv_layout, self._paged_kv_indptr_buf, self._paged_kv_indices_buf,
            self._paged_kv_last_page_len_buf, self._batch_size)
        pos_encoding_mode = self._pos_encoding_mode
        _check_pos_encoding_mode(pos_encoding_mode)
        if q.dim() != 3 or q.shape[0] != self._batch_size or q.shape[1] != self._num_qo_heads:
            raise ValueError(
                f"q must have shape [{self._batch_size}, {self._num_qo_heads}, head_dim], got {tuple(q.shape)}"
            )
        if q.shape[2] != head_dim or head_dim != self._head_dim:
            raise ValueError("head_dim of q / kv cache does not match the planned head_dim")
        if num_kv_heads != self._num_kv_heads or page_size != self._page_size:
            raise ValueError("kv cache shape does not match the planned num_kv_heads / page_size")
        if q.stride(-1) != 1:
            raise ValueError("q must be contiguous in head_dim")
        if lse is not None:
            check_shape_dtype_device(lse, (q.size(0), q.size(1)), torch.float32, q.device, "lse")
        check_shape_dtype_device(out, q.shape, q.dtype, q.device, "out")
        if not out.is_contiguous():
            raise ValueError("out must be contiguous")
        alibi = None
        if pos_encoding_mode == "ALIBI":
            alibi = _get_cache_alibi_slopes_buf(q.shape[1], q.device)
        params = _lib.fi_batch_decode_params_t(
            q=q.data_ptr(), q_stride_n=q.stride(0), q_stride_h=q.stride(1),
            kv=kv,
            o=out.data_ptr(), lse=_lib.ptr(lse),
            alibi_slopes=_lib.ptr(alibi), q_rope_offset=None, num_qo_heads=self._num_qo_heads,
            q_dtype=_lib.fi_dtype(q.dtype), pos_encoding_mode=PosEncodingMode[pos_encoding_mode].value,
            window_left=self._window_left,
            **_resolve_logits_params(q.shape[-1], self._sm_scale, q_scale, k_scale, self._logits_soft_cap,
                                     self._rope_scale, self._rope_theta),
        )
        self._fws_ptr, self._fws_bytes, self._iws_ptr, self._iws_bytes = self._workspace_args
        self._lib_run = _lib.lib().fi_batch_decode_run
        self._lib_run_sinks = _lib.lib().fi_batch_decode_run_sinks
        return C.byref(params)

    def forward_return_lse(
        self,
        q: torch.Tensor,
        paged_kv_cache: torch.Tensor,
        pos_encoding_mode: str = "NONE",
        q_scale: Optional[float] = None,
        k_scale: Optional[float] = None,
        v_scale: Optional[float] = None,
        window_left: int = -1,
        logits_soft_cap: Optional[float] = None,
        sm_scale: Optional[float] = None,
        rope_scale: Optional[float] = None,
        rope_theta: Optional[float] = None,
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        r"""Warning: this function is deprecated, please use :meth:`run_return_lse` instead."""
        self._set_run_options(pos_encoding_mode, window_left, logits_soft_cap, sm_scale, rope_scale, rope_theta)
        self._run_cache = None
        return self.run(
            q, paged_kv_cache, q_scale=q_scale, k_scale=k_scale, v_scale=v_scale, return_lse=True
        )

    run_return_lse = functools.partialmethod(run, return_lse=True)

    def end_forward(self) -> None:
        r"""Warning: this function is deprecated and has no effect."""
        pass


class CUDAGraphBatchDecodeWithPagedKVCacheWrapper(BatchDecodeWithPagedKVCacheWrapper):
    r"""Graph-capturable batch decode wrapper (hipGraph on ROCm): fixed batch size and launch shape.
    (ref: flashinfer/decode.py:1413-1480)"""

    def __init__(
        self,
        workspace_buffer: torch.Tensor,
        indptr_buffer: torch.Tensor,
        indices_buffer: torch.Tensor,
        last_page_len_buffer: torch.Tensor,
        kv_layout: str = "NHD",
        use_tensor_cores: bool = False,
    ) -> None:
        super().__init__(
            workspace_buffer,
            kv_layout,
            use_cuda_graph=True,
            use_tensor_cores=use_tensor_cores,
            paged_kv_indptr_buffer=indptr_buffer,
            paged_kv_indices_buffer=indices_buffer,
            paged_kv_last_page_len_buffer=last_page_len_buffer,
        )


def trtllm_batch_decode_with_kv_cache(
    query: torch.Tensor,
    kv_cache: Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]],
    workspace_buffer: torch.Tensor,
    block_tables: torch.Tensor,
    seq_lens: torch.Tensor,
    max_seq_len: int,
    bmm1_scale: float,
    bmm2_scale: float,
    window_left: int = -1,
    out: Optional[torch.Tensor] = None,
    out_dtype: Optional[Union[torch.dtype, str]] = None,
    o_sf_scale: Optional[float] = None,
    o_sf_vec_size: Optional[int] = None,
    sinks: Optional[List[torch.Tensor]] = None,
    enable_pdl: bool = None,
    q_len_per_req: Optional[int] = 1,
) -> torch.Tensor:
    r"""Plan-free batch decode over a paged KV cache (ref: flashinfer/decode.py:2054-2071): a dense block table and
    device-resident lengths instead of ``plan()``.  The split-KV work list is built by kernels on the current stream
    (fi_batch_decode_plan_device), then the kernels of :class:`BatchDecodeWithPagedKVCacheWrapper` run on it.  There
    is no host synchronisation and no allocation that depends on a length, so the whole call can be captured in a
    graph; a replay plans again from what ``block_tables`` and ``seq_lens`` hold then.

    query : ``[batch_size, num_qo_heads, head_dim]``, float16 or bfloat16.
    kv_cache : one tensor ``[num_pages, 2, num_kv_heads, page_size, head_dim]`` (the HND layout), or a ``(k, v)`` tuple
        of ``[num_pages, num_kv_heads, page_size, head_dim]`` tensors.
    workspace_buffer : one buffer on the query's device; the work list, the page table and the f32 partial states are
        carved out of it.  It need not be zeroed.  ValueError names the bytes needed when it is too small.
    block_tables : int32 ``[batch_size, max_blocks]``; row ``b`` lists the pages of request ``b``.  Entries past a
        request's ``ceil(seq_len / page_size)`` pages are never read.
    seq_lens : int32 (or uint32) ``[batch_size]`` on the device.  A length beyond ``max_blocks * page_size`` is CLAMPED
        to it (the host never sees the value, so it cannot be refused); a length of 0 gives a zero output row.
    max_seq_len : checked against ``max_blocks * page_size``; otherwise unused.
    bmm1_scale : the full scale of the logits (``sm_scale``).  bmm2_scale : multiplies the output.
    window_left : sliding window, ``-1`` for none.  Chunks are cut over all pages; the kernel masks.
    out : optional output tensor of the query's shape and dtype.  out_dtype : the query's dtype, if given.
    sinks : optional float32 ``[num_qo_heads]`` attention-sink logits (or a one-element list holding them).
    enable_pdl : accepted and ignored.

    Not offered (NotImplementedError): ``q_len_per_req != 1``, an fp8 query, ``out_dtype="nvfp4"`` / an FP4Tensor
    ``out`` / ``o_sf_scale`` / ``o_sf_vec_size``, and the ``[num_pages, 1, ...]`` cache with K and V shared.
    """
    if q_len_per_req is not None and q_len_per_req != 1:
        raise NotImplementedError(f"trtllm_batch_decode_with_kv_cache: q_len_per_req={q_len_per_req} is not "
                                  "supported (one query token per request)")
    if query.dtype in (torch.float8_e4m3fn, torch.float8_e5m2):
        raise NotImplementedError("trtllm_batch_decode_with_kv_cache: an fp8 query is not supported "
                                  "(float16 / bfloat16)")
    _refuse_fp4_out_and_shared_kv("trtllm_batch_decode_with_kv_cache", kv_cache, out, out_dtype, o_sf_scale,
                                  o_sf_vec_size)
    for name, t in (("query", query), ("workspace_buffer", workspace_buffer), ("block_tables", block_tables),
                    ("seq_lens", seq_lens)):
        _lib.require_gpu_tensor(t, name)
    k_cache, v_cache = _hnd_cache_views(kv_cache)
    if query.dtype not in (torch.float16, torch.bfloat16) or query.dim() != 3 or query.stride(-1) != 1:
        raise ValueError("query must be a float16 / bfloat16 [batch_size, num_qo_heads, head_dim] tensor, contiguous "
                         "in head_dim")
    batch_size, num_qo_heads, head_dim = query.shape
    seq_lens = _check_block_tables_and_lens(block_tables, seq_lens, workspace_buffer, batch_size)
    if out_dtype is not None and canonicalize_torch_dtype(out_dtype) != query.dtype:
        raise ValueError(f"out_dtype {out_dtype} differs from the query's {query.dtype}")
    out = _out_or_empty(out, query.shape, query.dtype, query.device)
    sinks = _one_sinks_tensor(sinks, num_qo_heads, query.device)

    max_blocks = block_tables.shape[1]
    # the cache view; its three page-table pointers are set below, once the planner has said where it writes them
    kv, page_size, num_kv_heads, kv_head_dim = paged_kv(k_cache, v_cache, "HND", block_tables, None, None, batch_size)
    if kv_head_dim != head_dim:
        raise ValueError(f"head_dim of query ({head_dim}) and kv_cache ({kv_head_dim}) differ")
    _check_len_fits_block_tables("max_seq_len", max_seq_len, max_blocks, page_size)
    if batch_size == 0:
        return out

    plan = _lib.fi_batch_decode_plan_device_params_t(
        block_tables=block_tables.data_ptr(), seq_lens=seq_lens.data_ptr(), block_tables_stride=block_tables.stride(0),
        batch_size=batch_size, max_blocks=max_blocks, page_size=page_size, num_qo_heads=num_qo_heads,
        num_kv_heads=num_kv_heads, head_dim=head_dim, q_dtype=_lib.fi_dtype(query.dtype),
        kv_dtype=_lib.fi_dtype(k_cache.dtype), max_grid_hint=0)
    _device_plan_regions(workspace_buffer, plan, "fi_batch_decode_plan_device_workspace",
                         "trtllm_batch_decode_with_kv_cache")
    plan_info = (C.c_int64 * _lib.FI_DECODE_PLAN_INFO_LEN)()
    csr = (C.c_int64 * 3)()
    params = _lib.fi_batch_decode_params_t(
        q=query.data_ptr(), q_stride_n=query.stride(0), q_stride_h=query.stride(1), kv=kv, o=out.data_ptr(), lse=None,
        alibi_slopes=None, q_rope_offset=None, num_qo_heads=num_qo_heads, q_dtype=plan.q_dtype,
        pos_encoding_mode=PosEncodingMode.NONE.value, window_left=window_left,
        **_resolve_logits_params(head_dim, bmm1_scale, None, None, None, None, None))
    lib = _lib.lib()
    with torch.cuda.device(query.device):
        stream = _lib.current_stream(query.device)
        _lib.check(lib.fi_batch_decode_plan_device(C.byref(plan), plan_info, csr, stream),
                   "trtllm_batch_decode_with_kv_cache")
        # the page table the planner's kernels write, in place of the one plan() would have been given
        params.kv.indptr, params.kv.indices, params.kv.last_page_len = (plan.int_ws + off for off in csr)
        _lib.check(lib.fi_batch_decode_run_sinks(plan.float_ws, plan.float_ws_bytes, plan.int_ws, plan.int_ws_bytes,
                                                 plan_info, _lib.FI_DECODE_PLAN_INFO_LEN, C.byref(params),
                                                 _lib.ptr(sinks), stream),
                   "trtllm_batch_decode_with_kv_cache")
    if bmm2_scale != 1.0:
        out *= bmm2_scale
    return out


def _mla_query_rows(query: torch.Tensor) -> int:
    """The element stride between consecutive query tokens of ``[batch, q_len, num_heads, 576]`` flattened to
    ``[batch * q_len, num_heads, 576]`` without a copy; ValueError when the tensor cannot be read that way."""
    batch_size, q_len = query.shape[:2]
    if query.stride(-1) != 1:
        raise ValueError("query must be contiguous in its last dimension")
    if q_len > 1 and batch_size > 1 and query.stride(0) != q_len * query.stride(1):
        raise ValueError("query must flatten to [batch_size * q_len_per_request, num_heads, 576] without a copy: "
                         f"stride(0) = {query.stride(0)} is not q_len_per_request x stride(1) = "
                         f"{q_len} x {query.stride(1)}")
    stride_n = query.stride(1) if q_len > 1 else query.stride(0)
    per16 = 16 // query.element_size()  # elements in 16 bytes: 8 at 16 bit, 16 for fp8
    if stride_n % per16 or query.stride(2) % per16 or query.data_ptr() % 16:
        raise ValueError(f"query: strides must be multiples of {per16} elements and the base 16-byte aligned")
    return stride_n


def trtllm_batch_decode_with_kv_cache_mla(
    query: torch.Tensor,
    kv_cache: torch.Tensor,
    workspace_buffer: torch.Tensor,
    qk_nope_head_dim: int,
    kv_lora_rank: int,
    qk_rope_head_dim: int,
    block_tables: torch.Tensor,
    seq_lens: torch.Tensor,
    max_seq_len: int,
    out: Optional[torch.Tensor] = None,
    bmm1_scale: Optional[float] = 1.0,
    bmm2_scale: Optional[float] = 1.0,
    bmm1_scale_log2_tensor: Optional[torch.Tensor] = None,
    bmm2_scale_tensor: Optional[torch.Tensor] = None,
    sinks: Optional[List[torch.Tensor]] = None,
    enable_pdl: bool = None,
) -> torch.Tensor:
    r"""Plan-free MLA decode over a paged cache (ref: flashinfer/decode.py:2298-2315): a dense block table and
    device-resident lengths instead of ``BatchMLAPagedAttentionWrapper.plan()``.  The work list is built by kernels on
    the current stream (fi_batch_mla_plan_device), then the kernel of
    :class:`flashinfer.mla.BatchMLAPagedAttentionWrapper` runs on it.  There is no host synchronisation and no
    allocation that depends on a length, so the whole call can be captured in a graph; a replay plans again from what
    ``block_tables`` and ``seq_lens`` hold then.

    query : ``[batch_size, q_len_per_request, num_heads, 576]`` (``q_nope | q_pe``), float16, bfloat16 or float8_e4m3fn,
        contiguous in the last dimension and flattenable to ``[batch_size * q_len_per_request, num_heads, 576]`` without
        a copy; strides multiples of 8 elements (16 for fp8), the base 16-byte aligned.  ``q_len_per_request > 1`` (MTP, speculative
        verify) is causal within the request: row ``i`` sees keys ``<= seq_len - q_len_per_request + i``, and a row
        that sees no key gives zeros.
    kv_cache : ``[num_pages, 1, page_size, 576]`` or ``[num_pages, page_size, 576]`` (``ckv | kpe``), of the query's
        dtype; strides multiples of 8 elements (16 for fp8).  Query and cache are both 16-bit or both float8_e4m3fn, as
        :func:`flashinfer.rope.mla_rope_quantize_fp8` and an fp8 :func:`flashinfer.page.append_paged_mla_kv_cache`
        leave them; the fp8 bytes are upcast exactly to bfloat16 while they are staged, and the kernel from there on is
        the bfloat16 one.  Any page size is taken: the reference's 32 / 64 restriction and its ``block_num % (128 / block_size)``
        rule are tile constraints of its kernels and are not enforced here.
    workspace_buffer : one buffer on the query's device; the work list and the f32 partial states are carved out of
        it.  It need not be zeroed.  ValueError names the bytes needed when it is too small; whatever it holds beyond
        that goes to partial states, and a small buffer only makes the planner cut longer chunks.
    qk_nope_head_dim, kv_lora_rank, qk_rope_head_dim : 128, 512, 64; anything else is a ValueError.
    block_tables : int32 ``[batch_size, max_blocks]``; row ``b`` lists the pages of request ``b``.  Entries past a
        request's ``ceil(seq_len / page_size)`` pages are never read.
    seq_lens : int32 (or uint32) ``[batch_size]`` on the device.  A length beyond ``max_blocks * page_size`` is CLAMPED
        to it (the host never sees the value, so it cannot be refused); a length of 0 gives zero output rows.
    max_seq_len : checked against ``max_blocks * page_size``; otherwise unused.
    out : optional ``[batch_size, q_len_per_request, num_heads, 512]``, or ``[batch_size, num_heads, 512]`` when
        ``q_len_per_request == 1``, contiguous, of the query's dtype (bfloat16 for an fp8 query, as the reference
        allocates); allocated in the first form when not given.
    bmm1_scale : the full scale of the logits; with fp8 tensors the caller folds ``q_scale * k_scale`` into it (as the
        reference: ``q_scale * k_scale * sm_scale``).  bmm2_scale : multiplies the output (``v_scale * o_scale``).
    bmm1_scale_log2_tensor, bmm2_scale_tensor : with an fp8 query and cache only, and only both together: float32
        tensors of one element on the query's device, which take precedence over the floats, as in the reference.  The
        first is the logit scale times log2(e), read by the kernel; the second multiplies the output on the device.
        Neither is read on the host, so a captured call follows them when they change in place.
    enable_pdl : accepted and ignored.

    Not offered (NotImplementedError): an fp8 query with a 16-bit cache or a 16-bit query with an fp8 cache, float8_e5m2,
    ``bmm1_scale_log2_tensor`` / ``bmm2_scale_tensor`` with a 16-bit query or one without the other, and ``sinks``.
    """
    name = "trtllm_batch_decode_with_kv_cache_mla"
    fp8 = (torch.float8_e4m3fn, torch.float8_e5m2)
    if torch.float8_e5m2 in (query.dtype, kv_cache.dtype):
        raise NotImplementedError(f"{name}: a float8_e5m2 (e5m2) fp8 query or kv_cache is not supported (fp8 is "
                                  "float8_e4m3fn)")
    if (query.dtype in fp8) != (kv_cache.dtype in fp8):
        raise NotImplementedError(f"{name}: an fp8 query or kv_cache needs the other to be fp8 too; a mixed pair "
                                  f"({query.dtype} query, {kv_cache.dtype} kv_cache) is not supported")
    is_fp8 = query.dtype in fp8
    given = [n for n, t in (("bmm1_scale_log2_tensor", bmm1_scale_log2_tensor),
                            ("bmm2_scale_tensor", bmm2_scale_tensor)) if t is not None]
    if given and not is_fp8:
        raise NotImplementedError(f"{name}: {' / '.join(given)} with a 16-bit query is not supported (pass bmm1_scale "
                                  "/ bmm2_scale as floats)")
    if len(given) == 1:
        raise NotImplementedError(f"{name}: {given[0]} alone is not supported: give bmm1_scale_log2_tensor and "
                                  "bmm2_scale_tensor together")
    if sinks is not None:
        raise NotImplementedError(f"{name}: sinks are not supported")
    if (qk_nope_head_dim, kv_lora_rank, qk_rope_head_dim) != (128, 512, 64):
        raise ValueError(f"{name}: qk_nope_head_dim / kv_lora_rank / qk_rope_head_dim must be 128 / 512 / 64, got "
                         f"{qk_nope_head_dim} / {kv_lora_rank} / {qk_rope_head_dim}")
    for what, t in (("query", query), ("kv_cache", kv_cache), ("workspace_buffer", workspace_buffer),
                    ("block_tables", block_tables), ("seq_lens", seq_lens)):
        _lib.require_gpu_tensor(t, what)
    head_dim = kv_lora_rank + qk_rope_head_dim
    if query.dtype not in (torch.float16, torch.bfloat16, torch.float8_e4m3fn) or query.dim() != 4 \
            or query.shape[-1] != head_dim:
        raise ValueError(f"query must be a float16 / bfloat16 / float8_e4m3fn [batch_size, q_len_per_request, "
                         f"num_heads, {head_dim}] tensor")
    for what, t in (("bmm1_scale_log2_tensor", bmm1_scale_log2_tensor), ("bmm2_scale_tensor", bmm2_scale_tensor)):
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32 or t.numel() != 1
                              or t.device != query.device):
            raise ValueError(f"{what} must be a float32 tensor of one element on the query's device")
    batch_size, q_len, num_heads, _ = query.shape
    if q_len == 0 or num_heads == 0:
        raise ValueError("query must hold at least one token per request and one head")
    q_stride_n = _mla_query_rows(query)
    if kv_cache.dim() == 4 and kv_cache.shape[1] == 1:
        kv_cache = kv_cache.squeeze(1)
    if kv_cache.dim() != 3 or kv_cache.shape[-1] != head_dim or kv_cache.dtype != query.dtype \
            or kv_cache.stride(-1) != 1:
        raise ValueError(f"kv_cache must be [num_pages, 1, page_size, {head_dim}] or [num_pages, page_size, {head_dim}]"
                         f", of the query's dtype {query.dtype} and contiguous in the last dimension")
    per16 = 16 // kv_cache.element_size()
    if kv_cache.stride(0) % per16 or kv_cache.stride(1) % per16 or kv_cache.data_ptr() % 16:
        raise ValueError(f"kv_cache: strides must be multiples of {per16} elements and the base 16-byte aligned")
    page_size = kv_cache.shape[1]
    seq_lens = _check_block_tables_and_lens(block_tables, seq_lens, workspace_buffer, batch_size)
    max_blocks = block_tables.shape[1]
    _check_len_fits_block_tables("max_seq_len", max_seq_len, max_blocks, page_size)
    if batch_size * block_tables.stride(0) >= 1 << 31:
        raise ValueError("batch_size x block_tables.stride(0) must be below 2^31")
    out_shape = (batch_size, q_len, num_heads, kv_lora_rank)
    if out is not None and q_len == 1 and out.dim() == 3:
        out_shape = (batch_size, num_heads, kv_lora_rank)
    # an fp8 query computes in bf16 and writes bf16, as the reference allocates
    compute_dtype = torch.bfloat16 if is_fp8 else query.dtype
    out = _out_or_empty(out, out_shape, compute_dtype, query.device)
    if batch_size == 0:
        return out

    # a plan is cut from lengths alone: the planner is given the compute dtype, run() the storage types
    dtype = _lib.fi_dtype(compute_dtype)
    storage = _lib.FI_DTYPE_FP8_E4M3 if is_fp8 else 0
    plan = _lib.fi_batch_mla_plan_device_params_t(
        block_tables=block_tables.data_ptr(), seq_lens=seq_lens.data_ptr(), block_tables_stride=block_tables.stride(0),
        batch_size=batch_size, max_blocks=max_blocks, page_size=page_size, num_heads=num_heads,
        q_len_per_request=q_len, head_dim_ckv=kv_lora_rank, head_dim_kpe=qk_rope_head_dim, q_dtype=dtype,
        kv_dtype=dtype, max_items_hint=0)
    _device_plan_regions(workspace_buffer, plan, "fi_batch_mla_plan_device_workspace", name)
    plan_info = (C.c_int64 * _lib.FI_MLA_PLAN_INFO_LEN)()
    item = query.element_size()
    # q_nope / q_pe and ckv / kpe are views of the two 576-wide tensors
    params = _lib.fi_batch_mla_params_t(
        q_nope=query.data_ptr(), q_nope_stride_n=q_stride_n, q_nope_stride_h=query.stride(2),
        q_pe=query.data_ptr() + kv_lora_rank * item, q_pe_stride_n=q_stride_n, q_pe_stride_h=query.stride(2),
        ckv=kv_cache.data_ptr(), ckv_stride_page=kv_cache.stride(0), ckv_stride_n=kv_cache.stride(1),
        kpe=kv_cache.data_ptr() + kv_lora_rank * item, kpe_stride_page=kv_cache.stride(0),
        kpe_stride_n=kv_cache.stride(1),
        # no CSR page table: the planner's items address the block table's rows
        kv_indices=block_tables.data_ptr(), o=out.data_ptr(), lse=None,
        float_ws=plan.float_ws, float_ws_bytes=plan.float_ws_bytes, int_ws=plan.int_ws, int_ws_bytes=plan.int_ws_bytes,
        num_rows=batch_size * q_len * num_heads, num_heads=num_heads, page_size=page_size, dtype=dtype, causal=1,
        sm_scale=1.0 if bmm1_scale is None else float(bmm1_scale), q_fp8=storage, kv_fp8=storage,
        sm_scale_log2_dev=_lib.ptr(bmm1_scale_log2_tensor))
    lib = _lib.lib()
    with torch.cuda.device(query.device):
        stream = _lib.current_stream(query.device)
        _lib.check(lib.fi_batch_mla_plan_device(C.byref(plan), plan_info, stream), name)
        _lib.check(lib.fi_batch_mla_run(plan_info, _lib.FI_MLA_PLAN_INFO_LEN, C.byref(params), stream), name)
    if bmm2_scale_tensor is not None:
        # on the device, no host read; in float32 and rounded once, as `out *= bmm2_scale` does with the float
        out.copy_(out.float().mul_(bmm2_scale_tensor.reshape(())))
    elif bmm2_scale is not None and bmm2_scale != 1.0:
        out *= bmm2_scale
    return out
