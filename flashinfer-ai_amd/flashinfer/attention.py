"""``BatchAttentionWithAttentionSinkWrapper``: paged prefill / append / decode attention with per-head attention sinks,
the front-end GPT-OSS style models call (ref: flashinfer/attention.py:201-275).

A sink is one logit per query head that joins the softmax denominator of every row and has no value vector
(ref: AttentionSink, flashinfer/jit/attention/variants.py:17-53).  The kernels are the paged prefill kernels
(csrc/prefill_kernel.h); the sink is folded where they write a final output row, or in the merge launch of a split-KV
plan -- no extra launch.
"""
from __future__ import annotations

from typing import Optional

import torch

from .prefill import BatchPrefillWithPagedKVCacheWrapper
from .utils import _check_pos_encoding_mode, canonicalize_torch_dtype


class BatchAttentionWithAttentionSinkWrapper(BatchPrefillWithPagedKVCacheWrapper):
    r"""Prefill and decode attention over a paged KV cache with attention sinks.

    ``plan`` is :meth:`BatchPrefillWithPagedKVCacheWrapper.plan`; ``run`` takes the sink tensor and the softmax scale
    positionally, as the reference's generated module does:

    >>> wrapper = flashinfer.BatchAttentionWithAttentionSinkWrapper(
    ...     workspace_buffer, "NHD", q_data_type=torch.bfloat16, kv_data_type=torch.bfloat16,
    ...     head_dim_qk=64, head_dim_vo=64, window_left=127)
    >>> wrapper.plan(qo_indptr, paged_kv_indptr, paged_kv_indices, paged_kv_last_page_len, num_qo_heads,
    ...              num_kv_heads, 64, page_size, causal=True, window_left=127, q_data_type=torch.bfloat16,
    ...              kv_data_type=torch.bfloat16)
    >>> o = wrapper.run(q, kv_cache, sink, sm_scale)   # sink: float32 [num_qo_heads]

    ``sink`` holds natural-log logits that are not multiplied by ``sm_scale``; ``-inf`` switches a head's sink off.
    The logsumexp of ``run_return_lse`` includes the sink: such a state must not be merged with others again.
    float16 / bfloat16 queries and equal head dims only.
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
        pos_encoding_mode: str = "NONE",
        use_fp16_qk_reduction: bool = False,
        q_data_type: torch.dtype = torch.bfloat16,
        kv_data_type: torch.dtype = torch.bfloat16,
        head_dim_qk: int = 128,
        head_dim_vo: int = 128,
        window_left: int = -1,
    ) -> None:
        r"""Parameters as the reference (flashinfer/attention.py:208-227).  The reference compiles a module for
        ``pos_encoding_mode``, the dtypes, the head dims and ``window_left`` here; the kernels of this build take all
        of them at ``plan()`` / ``run()``, so they are only checked."""
        _check_pos_encoding_mode(pos_encoding_mode)
        if canonicalize_torch_dtype(q_data_type) not in (torch.float16, torch.bfloat16):
            raise ValueError(f"attention sinks need float16 or bfloat16 queries (got {q_data_type})")
        if head_dim_qk != head_dim_vo:
            raise ValueError(f"attention sinks need head_dim_qk == head_dim_vo (got {head_dim_qk} / {head_dim_vo})")
        # the variant list the reference builds (flashinfer/attention.py:241-255): entry 11 names the variant; the
        # module name and the CUDA declaration have no meaning here
        jit_args = [None, q_data_type, kv_data_type, q_data_type, torch.int32, head_dim_qk, head_dim_vo, ["sink"],
                    ["float"], ["sm_scale"], ["double"], "AttentionSink", None]
        super().__init__(
            float_workspace_buffer, kv_layout, use_cuda_graph, qo_indptr_buf, paged_kv_indptr_buf,
            paged_kv_indices_buf, paged_kv_last_page_len_buf, custom_mask_buf, mask_indptr_buf, backend,
            jit_args=jit_args,
        )
