"""Multi-head Latent Attention (MLA, DeepSeek-V2/V3/R1) over a paged cache (ref: flashinfer/mla.py:85-420).

The absorbed form: one shared KV "head" whose keys are ``[ckv | kpe]`` (512 + 64 dims) and whose values are the
``ckv`` part alone.  Every backend name the reference accepts for this path (``auto`` / ``fa2`` / ``fa3``) runs the
one HIP kernel of ``csrc/mla.hip``; the planner splits long requests into kv chunks and merges their partial states.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple, Union

import torch

from . import _lib
from ._wrapper import BatchAttentionWrapper, refuses_sinks

_MLA_INT_WORKSPACE_BYTES = 8 * 1024 * 1024


def _last_dim_contiguous(t: torch.Tensor, name: str) -> None:
    if t.stride(-1) != 1:
        raise ValueError(f"{name} must have a contiguous last dimension")


class BatchMLAPagedAttentionWrapper(BatchAttentionWrapper):
    r"""Wrapper class for MLA PagedAttention on DeepSeek models, for decode, speculative verify and incremental
    prefill with the matrix-absorbed weights (ref: flashinfer/mla.py:85-420).

    ``head_dim_ckv = 512`` and ``head_dim_kpe = 64`` only; q float16 or bfloat16, the caches of q's dtype or
    ``float8_e4m3fn``.  An fp8 cache is upcast exactly to q's dtype while it is staged, so the arithmetic is that of
    the 16-bit kernel on ``cache.to(q.dtype)``.  There is no k_scale / v_scale argument: ``sm_scale`` is the full
    scale of the logits, so the caller folds k_scale into it (``sm_scale * k_scale``) and multiplies the output by
    v_scale.  An fp8 q is a ValueError here
    (:func:`flashinfer.decode.trtllm_batch_decode_with_kv_cache_mla` takes one).
    ``ckv_cache``: ``[num_pages, page_size, 512]``, ``kpe_cache``: ``[num_pages, page_size, 64]`` (3-D, or 4-D
    with a middle head axis of 1).  Only the last dimension of each input must be contiguous, so views of one
    576-wide tensor (``q[..., :512]`` / ``q[..., 512:]``) are taken as they are.  ``lse`` is base 2.

    With ``use_cuda_graph=True`` plan() copies the page table into the buffers given here, and run() launches a
    fixed grid whose work list is read from the workspace, so a captured run() stays valid across plans for the
    same batch size, query count and head count; plan() refuses a change of any of them.
    """

    def __init__(
        self,
        float_workspace_buffer: torch.Tensor,
        use_cuda_graph: bool = False,
        qo_indptr: Optional[torch.Tensor] = None,
        kv_indptr: Optional[torch.Tensor] = None,
        kv_indices: Optional[torch.Tensor] = None,
        kv_len_arr: Optional[torch.Tensor] = None,
        backend: str = "auto",
    ) -> None:
        # of the reference's backend names only "cutlass" is refused: the others all run the one HIP kernel
        super().__init__(float_workspace_buffer, use_cuda_graph, backend, ("auto", "fa2", "fa3"),
                         int_workspace_bytes=_MLA_INT_WORKSPACE_BYTES)
        if use_cuda_graph:
            for t, name in ((qo_indptr, "qo_indptr"), (kv_indptr, "kv_indptr"), (kv_indices, "kv_indices"),
                            (kv_len_arr, "kv_len_arr")):
                if t is None:
                    raise ValueError(f"use_cuda_graph=True needs the {name} buffer")
            self._fixed_batch_size = qo_indptr.numel() - 1
        self._qo_indptr_buf = qo_indptr
        self._kv_indptr_buf = kv_indptr
        self._kv_indices_buf = kv_indices
        self._kv_len_arr_buf = kv_len_arr
        self._graph_rows = None  # (qo_indptr[-1], num_heads) of the first graph plan

    def plan(
        self,
        qo_indptr: torch.Tensor,
        kv_indptr: torch.Tensor,
        kv_indices: torch.Tensor,
        kv_len_arr: torch.Tensor,
        num_heads: int,
        head_dim_ckv: int,
        head_dim_kpe: int,
        page_size: int,
        causal: bool,
        sm_scale: float,
        q_data_type: torch.dtype,
        kv_data_type: torch.dtype,
        use_profiler: bool = False,
    ) -> None:
        r"""Plan the MLA attention of a batch (ref: flashinfer/mla.py:219-317).

        qo_indptr ``[batch + 1]``, kv_indptr ``[batch + 1]`` (pages), kv_indices ``[kv_indptr[-1]]``,
        kv_len_arr ``[batch]`` (tokens), all int32.  ``causal`` aligns query rows to the end of the sequence.
        """
        if use_profiler:
            raise ValueError("BatchMLAPagedAttentionWrapper: the profiler is not available on MI355X")
        if q_data_type not in (torch.float16, torch.bfloat16):
            raise ValueError(f"BatchMLAPagedAttentionWrapper: q_data_type must be float16 or bfloat16, got {q_data_type} "
                             "(an fp8 query is taken by trtllm_batch_decode_with_kv_cache_mla only)")
        if kv_data_type not in (q_data_type, torch.float8_e4m3fn):
            raise ValueError(f"BatchMLAPagedAttentionWrapper: kv_data_type must be q_data_type ({q_data_type}) or "
                             f"float8_e4m3fn, got {kv_data_type}")
        qo_indptr_host = qo_indptr.to("cpu").contiguous()
        kv_indptr_host = kv_indptr.to("cpu").contiguous()
        kv_len_arr_host = kv_len_arr.to("cpu").contiguous()
        batch_size = qo_indptr_host.numel() - 1
        if kv_indptr_host.numel() != batch_size + 1 or kv_len_arr_host.numel() != batch_size:
            raise ValueError("qo_indptr, kv_indptr and kv_len_arr disagree on the batch size")
        if self._use_cuda_graph:
            # a captured run() holds the q / out tensors and the merge launch of the first plan's packed row count
            # (qo_indptr[-1] x num_heads), and the workspace layout moves with it: every later plan must keep both
            graph_rows = (int(qo_indptr_host[-1]), int(num_heads))
            if self._graph_rows is not None and graph_rows != self._graph_rows:
                raise ValueError(
                    "use_cuda_graph: the query count and num_heads cannot change between plans "
                    f"(qo_indptr[-1], num_heads = {graph_rows}; first plan {self._graph_rows})"
                )
        self._bind_index_tensors(batch_size, True, prefix=("kv_indices",), qo_indptr=qo_indptr, kv_indptr=kv_indptr,
                                 kv_indices=kv_indices, kv_len_arr=kv_len_arr)
        params = _lib.fi_batch_mla_plan_params_t(
            int_ws=self._int_workspace_buffer.data_ptr(),
            pinned_int_ws=self._pin_memory_int_workspace_buffer.data_ptr(),
            int_ws_bytes=_lib.nbytes(self._int_workspace_buffer),
            float_ws_bytes=_lib.nbytes(self._float_workspace_buffer),
            qo_indptr_h=qo_indptr_host.data_ptr(), kv_indptr_h=kv_indptr_host.data_ptr(),
            kv_len_arr_h=kv_len_arr_host.data_ptr(), batch_size=batch_size, num_heads=num_heads,
            head_dim_ckv=head_dim_ckv, head_dim_kpe=head_dim_kpe, page_size=page_size, causal=int(bool(causal)),
            # a plan is cut from lengths alone: the planner is given the compute dtype for both, run() the storage type
            q_dtype=_lib.fi_dtype(q_data_type), kv_dtype=_lib.fi_dtype(q_data_type),
            enable_cuda_graph=int(bool(self._use_cuda_graph)), fixed_split_size=0,
        )
        info = (C.c_int64 * _lib.FI_MLA_PLAN_INFO_LEN)()
        with torch.cuda.device(self.device):
            _lib.check(
                _lib.lib().fi_batch_mla_plan(C.byref(params), info, _lib.current_stream(self.device)),
                "BatchMLAPagedAttentionWrapper.plan",
            )
        self._plan_info = info
        if self._use_cuda_graph and self._graph_rows is None:
            self._graph_rows = graph_rows
        self._num_heads = num_heads
        self._page_size = page_size
        self._causal = bool(causal)
        self._sm_scale = float(sm_scale)
        self._q_data_type = q_data_type
        self._kv_data_type = kv_data_type

    @refuses_sinks
    def run(
        self,
        q_nope: torch.Tensor,
        q_pe: torch.Tensor,
        ckv_cache: torch.Tensor,
        kpe_cache: torch.Tensor,
        out: Optional[torch.Tensor] = None,
        lse: Optional[torch.Tensor] = None,
        return_lse: bool = False,
        profiler_buffer: Optional[torch.Tensor] = None,
        kv_len: Optional[torch.Tensor] = None,
        page_table: Optional[torch.Tensor] = None,
    ) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        r"""Run the planned MLA attention (ref: flashinfer/mla.py:345-420).

        q_nope ``[nnz_qo, num_heads, 512]``, q_pe ``[nnz_qo, num_heads, 64]``; returns ``o`` of q_nope's shape
        and dtype, and with ``return_lse`` also ``lse`` ``[nnz_qo, num_heads]`` float32 (base 2).  With an fp8
        cache the strides of ckv_cache / kpe_cache are multiples of 16 elements and ``o`` is not yet multiplied by
        v_scale (see the class docstring).
        """
        if profiler_buffer is not None:
            raise ValueError("BatchMLAPagedAttentionWrapper: profiler_buffer is not supported on MI355X")
        if kv_len is not None or page_table is not None:
            raise ValueError("BatchMLAPagedAttentionWrapper: the kv_len / page_table call form is the cutlass "
                             "backend's and is not supported on MI355X")
        self._check_run_args()
        for t, name in ((q_nope, "q_nope"), (q_pe, "q_pe"), (ckv_cache, "ckv_cache"), (kpe_cache, "kpe_cache")):
            _lib.require_gpu_tensor(t, name)
            _last_dim_contiguous(t, name)
        if q_nope.dtype != self._q_data_type or q_pe.dtype != self._q_data_type:
            raise ValueError(f"q_nope / q_pe must be {self._q_data_type}, as planned")
        if ckv_cache.dtype != self._kv_data_type or kpe_cache.dtype != self._kv_data_type:
            raise ValueError(f"ckv_cache / kpe_cache must be {self._kv_data_type}, as planned")
        H = self._num_heads
        if q_nope.dim() != 3 or q_nope.shape[1:] != (H, 512) or q_pe.shape != (q_nope.shape[0], H, 64):
            raise ValueError("q_nope must be [nnz, num_heads, 512] and q_pe [nnz, num_heads, 64]")
        ckv3, kpe3 = ckv_cache, kpe_cache
        if ckv3.dim() == 4:
            ckv3 = ckv3.squeeze(2)
        if kpe3.dim() == 4:
            kpe3 = kpe3.squeeze(2)
        if ckv3.dim() != 3 or ckv3.shape[1] != self._page_size or ckv3.shape[2] != 512:
            raise ValueError("ckv_cache must be [num_pages, page_size, 512]")
        if kpe3.dim() != 3 or kpe3.shape[:2] != ckv3.shape[:2] or kpe3.shape[2] != 64:
            raise ValueError("kpe_cache must be [num_pages, page_size, 64]")
        nnz = q_nope.shape[0]
        if out is None:
            out = torch.empty((nnz, H, 512), dtype=q_nope.dtype, device=q_nope.device)
        elif out.shape != (nnz, H, 512) or out.dtype != q_nope.dtype or not out.is_contiguous():
            raise ValueError("out must be a contiguous [nnz, num_heads, 512] tensor of q's dtype")
        if return_lse:
            if lse is None:
                lse = torch.empty((nnz, H), dtype=torch.float32, device=q_nope.device)
            elif lse.shape != (nnz, H) or lse.dtype != torch.float32 or not lse.is_contiguous():
                raise ValueError("lse must be a contiguous float32 [nnz, num_heads] tensor")
        float_ws, float_ws_bytes, int_ws, int_ws_bytes = self._workspace_args
        params = _lib.fi_batch_mla_params_t(
            q_nope=q_nope.data_ptr(), q_nope_stride_n=q_nope.stride(0), q_nope_stride_h=q_nope.stride(1),
            q_pe=q_pe.data_ptr(), q_pe_stride_n=q_pe.stride(0), q_pe_stride_h=q_pe.stride(1),
            ckv=ckv3.data_ptr(), ckv_stride_page=ckv3.stride(0), ckv_stride_n=ckv3.stride(1),
            kpe=kpe3.data_ptr(), kpe_stride_page=kpe3.stride(0), kpe_stride_n=kpe3.stride(1),
            kv_indices=self._kv_indices_buf.data_ptr(), o=out.data_ptr(),
            lse=None if not return_lse else lse.data_ptr(),
            float_ws=float_ws, float_ws_bytes=float_ws_bytes, int_ws=int_ws, int_ws_bytes=int_ws_bytes,
            num_rows=nnz * H, num_heads=H, page_size=self._page_size, dtype=_lib.fi_dtype(q_nope.dtype),
            causal=int(self._causal), sm_scale=self._sm_scale,
            kv_fp8=_lib.FI_DTYPE_FP8_E4M3 if ckv3.dtype == torch.float8_e4m3fn else 0,
        )
        with torch.cuda.device(q_nope.device):
            _lib.check(
                _lib.lib().fi_batch_mla_run(self._plan_info, _lib.FI_MLA_PLAN_INFO_LEN, C.byref(params),
                                            _lib.current_stream(q_nope.device)),
                "BatchMLAPagedAttentionWrapper.run",
            )
        return (out, lse) if return_lse else out
