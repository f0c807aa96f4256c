"""Block-sparse attention: ``BlockSparseAttentionWrapper`` (a BSR matrix of ``R x C`` blocks as the attention mask)
and ``VariableBlockSparseAttentionWrapper`` (a block map per kv head over blocks of varying size).

Same names, arguments and defaults as the reference's ``flashinfer/sparse.py`` (:40-62, :65-701, :704-1269).  A BSR
block row is one request of the paged kernels: ``qo_len = R``, ``page_size = C``, ``last_page_len = C``, and the BSR
``indptr`` / ``indices`` are the page table as they stand (ref :315-357, :436-478).  Both classes therefore hold a
paged wrapper and add no attention arithmetic; what is new on the device is the expansion of a block map into page
indices (csrc/sparse.hip).  ``backend`` accepts ``auto`` / ``fa2`` / ``fa3`` and means the same thing.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple, Union

import torch

from . import _lib
from .decode import BatchDecodeWithPagedKVCacheWrapper
from .prefill import BatchPrefillWithPagedKVCacheWrapper
from .utils import canonicalize_qkv_dtypes, canonicalize_torch_dtype, is_float8


def convert_bsr_mask_layout(mask: torch.Tensor, indptr: torch.Tensor) -> torch.Tensor:
    r"""Convert a mask from BSR data layout ``(nnz, R, C)`` to the flattened layout of the paged wrappers' custom mask:
    block row after block row, each as a row-major ``[R, blocks_in_row * C]`` matrix (ref: flashinfer/sparse.py:40-62).

    Parameters
    ----------
    mask : torch.Tensor
        A boolean mask tensor with shape ``(nnz, R, C)``.
    indptr : torch.Tensor
        The indptr tensor in BSR format.

    Returns
    -------
    flattened_mask : torch.Tensor
        A flattened mask tensor with shape ``(nnz * R * C,)``.
    """
    nnz, R, C = mask.shape
    dev = mask.device
    ptr = indptr.to(device=dev, dtype=torch.int64)
    blocks = ptr[1:] - ptr[:-1]
    row = torch.repeat_interleave(torch.arange(len(blocks), device=dev), blocks, output_size=nnz)
    # element (r, c) of block k, the j-th of its block row, goes to row r, column j * C + c of that row's matrix
    first = ptr[row] * (R * C) + (torch.arange(nnz, device=dev) - ptr[row]) * C
    width = blocks[row] * C
    dest = (first[:, None, None] + torch.arange(R, device=dev)[None, :, None] * width[:, None, None]
            + torch.arange(C, device=dev)[None, None, :])
    out = torch.empty((nnz * R * C,), dtype=mask.dtype, device=dev)
    out[dest.reshape(-1)] = mask.reshape(-1)
    return out


class _SparseAttentionWrapper:
    """What the two wrappers share: the paged prefill wrapper they run on and the workspace calls."""

    def __init__(self, float_workspace_buffer: torch.Tensor, backend: str) -> None:
        self._prefill = BatchPrefillWithPagedKVCacheWrapper(float_workspace_buffer, "NHD", backend=backend)
        self._decode: Optional[BatchDecodeWithPagedKVCacheWrapper] = None
        self._active = None  # the wrapper the last plan() planned
        self.device = self._prefill.device
        self._backend = backend

    def reset_workspace_buffer(
        self,
        float_workspace_buffer: torch.Tensor,
        int_workspace_buffer: torch.Tensor,
        vector_sparse_indices_buffer: Optional[torch.Tensor] = None,
        vector_sparse_indptr_buffer: Optional[torch.Tensor] = None,
    ) -> None:
        r"""Reset the workspace buffers (both on the device of the input tensors).  A plan made before the call is
        void.  The ``vector_sparse_*_buffer`` arguments are accepted and unused: the kernels here read the block
        indices directly."""
        self._prefill.reset_workspace_buffer(float_workspace_buffer, int_workspace_buffer)
        if self._decode is not None:
            self._decode.reset_workspace_buffer(float_workspace_buffer, int_workspace_buffer)
        self._active = None

    def _planned(self):
        if self._active is None:
            raise RuntimeError("plan() must be called before run()")
        return self._active

    def _set_forward_options(self, pos_encoding_mode, logits_soft_cap, sm_scale, rope_scale, rope_theta) -> None:
        w = self._planned()
        w._set_run_options(pos_encoding_mode, -1, logits_soft_cap, sm_scale, rope_scale, rope_theta)
        if w is self._decode:
            w._run_cache = None

    def end_forward(self) -> None:
        r"""Warning: This method is deprecated and has no effect."""
        pass


class BlockSparseAttentionWrapper(_SparseAttentionWrapper):
    r"""Attention with a block-sparse matrix (SciPy ``bsr_matrix`` layout, any block size ``(R, C)``) as the mask.

    >>> workspace_buffer = torch.empty(128 * 1024 * 1024, dtype=torch.uint8, device="cuda:0")
    >>> bsr_wrapper = flashinfer.BlockSparseAttentionWrapper(workspace_buffer)
    >>> # sparse mask: [[0, 0, 1], [1, 0, 1], [0, 1, 1]]
    >>> indptr = torch.tensor([0, 1, 3, 5], dtype=torch.int32, device="cuda:0")
    >>> indices = torch.tensor([2, 0, 2, 1, 2], dtype=torch.int32, device="cuda:0")
    >>> bsr_wrapper.plan(indptr, indices, 3, 3, 1, 1, num_qo_heads, num_kv_heads, head_dim)
    >>> o = bsr_wrapper.run(q, k, v)   # q [3, num_qo_heads, head_dim]; k, v [3, num_kv_heads, head_dim]

    Block row ``i`` attends to the KV rows of its blocks in the order ``indices`` lists them (which need not be
    sorted).  A block row without blocks returns ``o = 0``, ``lse = -5e4``.  There is no CUDA-graph mode.
    (ref: flashinfer/sparse.py:65-701)
    """

    def __init__(
        self,
        float_workspace_buffer: torch.Tensor,
        backend: str = "auto",
    ) -> None:
        r"""float_workspace_buffer : split-KV partial states live here (128 MB recommended), on the device of the
        inputs.  backend : ``auto`` / ``fa2`` / ``fa3``; all three run the same kernels."""
        super().__init__(float_workspace_buffer, backend)
        self.R: Optional[int] = None
        self.C: Optional[int] = None
        self.M: Optional[int] = None
        self.N: Optional[int] = None

    def plan(
        self,
        indptr: torch.Tensor,
        indices: torch.Tensor,
        M: int,
        N: int,
        R: int,
        C: int,
        num_qo_heads: int,
        num_kv_heads: int,
        head_dim: int,
        mask: Optional[torch.Tensor] = None,
        packed_mask: Optional[torch.Tensor] = None,
        causal: bool = False,
        pos_encoding_mode: str = "NONE",
        use_fp16_qk_reduction: bool = False,
        logits_soft_cap: Optional[float] = None,
        sm_scale: Optional[float] = None,
        rope_scale: Optional[float] = None,
        rope_theta: Optional[float] = None,
        q_data_type: Union[str, torch.dtype] = "float16",
        kv_data_type: Optional[Union[str, torch.dtype]] = None,
        o_data_type: Union[str, torch.dtype] = "float16",
        non_blocking: bool = True,
    ) -> None:
        r"""Plan block-sparse attention for the ``M x N`` mask whose ``R x C`` blocks ``indptr`` / ``indices`` list.

        indptr : int32 ``(MB + 1,)``, ``MB = ceil(M / R)``; indices : int32 ``(nnz,)``, each below ``N // C``.
        ``N`` must be a multiple of ``C``; the last block row holds ``M - (MB - 1) * R`` query rows.
        mask : optional bool ``(nnz, R, C)``, the inside of every block; it is brought to the flattened layout with
            :func:`convert_bsr_mask_layout` and the rows past ``M`` of the last block row are dropped.
        packed_mask : its packed form (``segment_packbits(..., "little")`` of the flattened, trimmed mask, one
            segment of ``qo_len * kv_len`` bits per block row); takes precedence over ``mask``.
        causal : row ``i`` of a block row with ``qo_len`` rows sees the first ``kv_len - qo_len + i + 1`` of its
            gathered KV rows; ignored when a mask is given.
        o_data_type : output dtype.  16-bit queries need the same output dtype; fp8 queries float16 or bfloat16.
        The remaining arguments are those of :meth:`BatchPrefillWithPagedKVCacheWrapper.plan`;
        ``use_fp16_qk_reduction`` is accepted and unused.

        ``R == 1`` without a mask and with 16-bit queries runs on the batch decode kernels, one block row being one
        decode request; everything else runs on the paged prefill kernels.  The reference sends ``R * group < 4`` to
        decode (flashinfer/sparse.py:370-374), which is sound for ``R == 1`` only: its decode batch has one query row
        per request, so the rows 2 ... R of a block row would be read as further requests.
        (ref: flashinfer/sparse.py:206-485)
        """
        q_data_type, kv_data_type = canonicalize_qkv_dtypes(q_data_type, kv_data_type)
        o_data_type = canonicalize_torch_dtype(o_data_type)
        M, N, R, C = int(M), int(N), int(R), int(C)
        if R <= 0 or C <= 0 or M < 0 or N < 0:
            raise ValueError(f"M, N must be non-negative and R, C positive, got {M}, {N}, {R}, {C}")
        if N % C != 0:
            raise ValueError(f"N = {N} must be divisible by C = {C}")
        if num_kv_heads <= 0 or num_qo_heads % num_kv_heads != 0:
            raise ValueError(f"num_qo_heads {num_qo_heads} must be a multiple of num_kv_heads {num_kv_heads}")
        num_blocks_row = len(indptr) - 1
        if num_blocks_row != -(-M // R):
            raise ValueError(f"indptr has {len(indptr)} entries, expected ceil(M / R) + 1 = {-(-M // R) + 1}")
        if q_data_type in (torch.float16, torch.bfloat16) and o_data_type != q_data_type:
            raise ValueError(f"o_data_type {o_data_type} must equal the 16-bit q_data_type {q_data_type}")
        indptr_host = indptr.to("cpu").to(torch.int32).contiguous()
        nnz = int(indptr_host[-1]) if num_blocks_row else 0
        if (num_blocks_row and int(indptr_host[0]) != 0) or bool((indptr_host[1:] < indptr_host[:-1]).any()) \
                or nnz > indices.numel():
            raise ValueError("indptr must start at 0, not decrease, and end within indices")
        if nnz and (int(indices[:nnz].min()) < 0 or int(indices[:nnz].max()) >= N // C):
            raise ValueError(f"indices out of bound: every block index must be in [0, N / C = {N // C})")

        qo_indptr_host = R * torch.arange(num_blocks_row + 1, dtype=torch.int32)
        qo_indptr_host[-1] = M
        # a block row without blocks has kv_len 0 (get_seq_lens would read its last_page_len as its length)
        kv_lens_host = (indptr_host[1:] - indptr_host[:-1]) * C
        last_block_len = torch.full((num_blocks_row,), C, dtype=torch.int32, device=self.device)
        indptr = indptr.to(torch.int32)
        indices = indices.to(torch.int32)

        if packed_mask is None and mask is not None:
            if mask.dim() != 3 or tuple(mask.shape) != (nnz, R, C):
                raise ValueError(f"mask must have shape (nnz, R, C) = ({nnz}, {R}, {C}), got {tuple(mask.shape)}")
            mask = convert_bsr_mask_layout(mask, indptr_host)
            # the last block row holds M - (MB - 1) * R rows; its rows are the tail of the flattened mask
            if num_blocks_row > 0:
                mask = mask[: mask.numel() - (num_blocks_row * R - M) * int(kv_lens_host[-1])]

        self.M, self.N, self.R, self.C = M, N, R, C
        self._num_qo_heads, self._num_kv_heads, self._head_dim = num_qo_heads, num_kv_heads, head_dim
        self._o_dtype = o_data_type
        self._active = None
        if R == 1 and mask is None and packed_mask is None and q_data_type in (torch.float16, torch.bfloat16):
            if self._decode is None:
                self._decode = BatchDecodeWithPagedKVCacheWrapper(self._prefill._float_workspace_buffer, "NHD")
            self._decode.plan(
                indptr, indices, last_block_len, num_qo_heads, num_kv_heads, head_dim, C,
                pos_encoding_mode=pos_encoding_mode, logits_soft_cap=logits_soft_cap, q_data_type=q_data_type,
                kv_data_type=kv_data_type, sm_scale=sm_scale, rope_scale=rope_scale, rope_theta=rope_theta,
                non_blocking=non_blocking, seq_lens=kv_lens_host, _indptr_host=indptr_host)
            self._active = self._decode
        else:
            self._prefill.plan(
                qo_indptr_host, indptr, indices, last_block_len, num_qo_heads, num_kv_heads, head_dim, C,
                custom_mask=mask, packed_custom_mask=packed_mask, causal=causal, pos_encoding_mode=pos_encoding_mode,
                sm_scale=sm_scale, logits_soft_cap=logits_soft_cap, rope_scale=rope_scale, rope_theta=rope_theta,
                q_data_type=q_data_type, kv_data_type=kv_data_type, non_blocking=non_blocking,
                seq_lens=kv_lens_host, o_data_type=o_data_type)
            self._active = self._prefill

    begin_forward = plan

    @property
    def _use_tensor_cores(self) -> bool:
        """True when the last plan() chose the paged prefill kernels, False for batch decode (ref attribute)."""
        return self._planned() is self._prefill

    def forward(
        self,
        q: torch.Tensor,
        k: torch.Tensor,
        v: torch.Tensor,
        scale_q: Optional[torch.Tensor] = None,
        scale_k: Optional[torch.Tensor] = None,
        scale_v: Optional[torch.Tensor] = None,
        pos_encoding_mode: str = "NONE",
        use_fp16_qk_reduction: bool = False,
        logits_soft_cap: Optional[float] = None,
        sm_scale: Optional[float] = None,
        rope_scale: Optional[float] = None,
        rope_theta: Optional[float] = None,
    ) -> torch.Tensor:
        r"""Warning: This method is deprecated, please use :meth:`run` instead."""
        self._set_forward_options(pos_encoding_mode, logits_soft_cap, sm_scale, rope_scale, rope_theta)
        return self.run(q, k, v, scale_q, scale_k, scale_v)

    def run(
        self,
        q: torch.Tensor,
        k: torch.Tensor,
        v: torch.Tensor,
        scale_q: Optional[torch.Tensor] = None,
        scale_k: Optional[torch.Tensor] = None,
        scale_v: Optional[torch.Tensor] = None,
        out: Optional[torch.Tensor] = None,
        lse: Optional[torch.Tensor] = None,
        return_lse: bool = False,
        enable_pdl: Optional[bool] = None,
    ) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        r"""Compute block-sparse attention between Q/K/V tensors.

        q : ``(M, num_qo_heads, head_dim)``; k, v : ``(N, num_kv_heads, head_dim)``, read in place as ``N / C`` pages
        of ``C`` rows when contiguous.
        scale_q / scale_k / scale_v : per-head scales ``[num_qo_heads]`` / ``[num_kv_heads]`` of fp8 (e4m3 / e5m2)
            q = k = v; a missing one is 1.  Unused for 16-bit inputs.
        out : ``(M, num_qo_heads, head_dim)`` of ``o_data_type``; lse : float32 ``(M, num_qo_heads)``; both optional.
        enable_pdl : accepted and unused.
        Returns the output, and with ``return_lse`` the base-2 logsumexp ``(M, num_qo_heads)``.
        (ref: flashinfer/sparse.py:513-697)
        """
        w = self._planned()
        for t, name in ((q, "q"), (k, "k"), (v, "v")):
            _lib.require_gpu_tensor(t, name)
        if tuple(q.shape) != (self.M, self._num_qo_heads, self._head_dim):
            raise ValueError(f"q must have shape ({self.M}, {self._num_qo_heads}, {self._head_dim}), "
                             f"got {tuple(q.shape)}")
        kv_shape = (self.N, self._num_kv_heads, self._head_dim)
        if tuple(k.shape) != kv_shape or tuple(v.shape) != kv_shape:
            raise ValueError(f"k and v must have shape {kv_shape}, got {tuple(k.shape)} / {tuple(v.shape)}")
        kv = (k.reshape(-1, self.C, *k.shape[-2:]), v.reshape(-1, self.C, *v.shape[-2:]))
        if w is self._decode:
            return w.run(q, kv, out=out, lse=lse, return_lse=return_lse)
        if not is_float8(q):
            scale_q = scale_k = scale_v = None
        return w.run(q, kv, out=out, lse=lse, return_lse=return_lse, scale_q=scale_q, scale_k=scale_k,
                     scale_v=scale_v)


class VariableBlockSparseAttentionWrapper(_SparseAttentionWrapper):
    r"""Block-sparse attention over blocks of varying size, with a block map of its own for every kv head (a group of
    qo heads shares the map of its kv head).

    >>> wrapper = flashinfer.VariableBlockSparseAttentionWrapper(workspace_buffer)
    >>> block_mask_map = torch.tensor([[[0, 0, 1], [1, 0, 1], [0, 1, 1]]], dtype=torch.bool, device="cuda:0")
    >>> block_row_sz = torch.tensor([[1, 2, 3]], dtype=torch.int32, device="cuda:0")
    >>> block_col_sz = torch.tensor([[3, 1, 2]], dtype=torch.int32, device="cuda:0")
    >>> wrapper.plan(block_mask_map, block_row_sz, block_col_sz, num_qo_heads, num_kv_heads, head_dim)
    >>> o = wrapper.run(q, k, v)   # q [num_qo_heads, 6, head_dim]; k, v [num_kv_heads, 6, head_dim]

    Every (kv head, block row) is one request of the paged prefill kernels over a cache of one kv head whose pages
    hold ``g`` tokens, ``g`` the greatest common divisor of all column sizes (the reference uses one-token pages
    throughout: uniform 128-wide blocks need 128 times fewer page indices here).  There is no CUDA-graph mode.
    (ref: flashinfer/sparse.py:704-1269)
    """

    def __init__(
        self,
        float_workspace_buffer: torch.Tensor,
        backend: str = "auto",
    ) -> None:
        r"""float_workspace_buffer : split-KV partial states live here (128 MB recommended), on the device of the
        inputs.  backend : ``auto`` / ``fa2`` / ``fa3``; all three run the same kernels."""
        super().__init__(float_workspace_buffer, backend)

    def plan(
        self,
        block_mask_map: torch.Tensor,
        block_row_sz: torch.Tensor,
        block_col_sz: torch.Tensor,
        num_qo_heads: int,
        num_kv_heads: int,
        head_dim: int,
        causal: bool = False,
        pos_encoding_mode: str = "NONE",
        use_fp16_qk_reduction: bool = False,
        logits_soft_cap: Optional[float] = None,
        sm_scale: Optional[float] = None,
        rope_scale: Optional[float] = None,
        rope_theta: Optional[float] = None,
        non_blocking: bool = True,
        q_data_type: Union[str, torch.dtype] = "float16",
        kv_data_type: Optional[Union[str, torch.dtype]] = None,
    ) -> None:
        r"""Plan attention for the block map.

        block_mask_map : ``(num_kv_heads, MB, NB)`` bool (or any integer type, non-zero = selected).
        block_row_sz : ``(num_kv_heads, MB)`` int, block_col_sz : ``(num_kv_heads, NB)`` int: the block sizes of every
            head.  Each head's row sizes must sum to the same ``qo_len`` and its column sizes to the same ``kv_len``.
        causal : row ``i`` of a block row with ``qo_len`` rows sees the first ``kv_len - qo_len + i + 1`` KV rows of
            its selected blocks.
        The remaining arguments are those of :meth:`BatchPrefillWithPagedKVCacheWrapper.plan`;
        ``use_fp16_qk_reduction`` is accepted and unused.

        The page indices are written on the device (fi_block_mask_row_pages, fi_block_mask_to_page_indices) and never
        visit the host; the ``num_kv_heads * MB + 1`` prefix sums do, for the planner.  A split-KV plan keeps one
        merge entry per query row in the 8 MB int workspace, so very large ``num_kv_heads * qo_len`` is refused by
        the planner with its own message.
        (ref: flashinfer/sparse.py:824-1076)
        """
        if block_mask_map.dim() != 3 or block_row_sz.dim() != 2 or block_col_sz.dim() != 2:
            raise ValueError("block_mask_map must be 3-D, block_row_sz and block_col_sz 2-D")
        H, MB, NB = block_mask_map.shape
        if H != num_kv_heads or tuple(block_row_sz.shape) != (H, MB) or tuple(block_col_sz.shape) != (H, NB):
            raise ValueError(
                f"block_mask_map {tuple(block_mask_map.shape)} must be (num_kv_heads = {num_kv_heads}, MB, NB) with "
                f"block_row_sz (num_kv_heads, MB) and block_col_sz (num_kv_heads, NB), got "
                f"{tuple(block_row_sz.shape)} / {tuple(block_col_sz.shape)}")
        if H == 0 or MB == 0 or NB == 0:
            raise ValueError(f"empty block map {tuple(block_mask_map.shape)}")
        if num_qo_heads % num_kv_heads != 0:
            raise ValueError(f"num_qo_heads {num_qo_heads} must be a multiple of num_kv_heads {num_kv_heads}")
        row_host = block_row_sz.to("cpu").to(torch.int64)
        col_host = block_col_sz.to("cpu").to(torch.int64)
        if int(row_host.min()) < 0 or int(col_host.min()) < 0:
            raise ValueError("block sizes must be non-negative")
        qo_lens, kv_lens = row_host.sum(1), col_host.sum(1)
        if bool((qo_lens != qo_lens[0]).any()) or bool((kv_lens != kv_lens[0]).any()):
            raise ValueError(f"every head's block sizes must sum to one length: row sums {qo_lens.tolist()}, column "
                             f"sums {kv_lens.tolist()}")
        qo_len, kv_len = int(qo_lens[0]), int(kv_lens[0])
        g = math.gcd(*col_host.flatten().tolist()) or 1  # the page size: divides every column block
        if H * (kv_len // g) >= 2 ** 31:
            raise ValueError(f"{H} heads x {kv_len // g} pages of {g} tokens do not fit int32 page numbers")

        dev = self.device
        mask = block_mask_map.to(dev)
        mask = (mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0).contiguous().view(torch.uint8)
        col_sz = block_col_sz.to(device=dev, dtype=torch.int32).contiguous()
        row_pages = torch.empty((H * MB,), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(
                _lib.lib().fi_block_mask_row_pages(mask.data_ptr(), col_sz.data_ptr(), H, MB, NB, g, kv_len,
                                                   row_pages.data_ptr(), _lib.current_stream(dev)),
                "VariableBlockSparseAttentionWrapper.plan")
        kv_indptr = torch.zeros((H * MB + 1,), dtype=torch.int64, device=dev)
        kv_indptr[1:] = torch.cumsum(row_pages, 0, dtype=torch.int64)
        kv_indptr_host = kv_indptr.to("cpu")
        num_pages = int(kv_indptr_host[-1])
        if num_pages >= 2 ** 31:
            raise ValueError(f"the block map selects {num_pages} pages of {g} tokens: the page table holds at most "
                             f"2^31 - 1")
        kv_indptr_host = kv_indptr_host.to(torch.int32)
        kv_indptr = kv_indptr.to(torch.int32)
        kv_indices = torch.empty((max(num_pages, 1),), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(
                _lib.lib().fi_block_mask_to_page_indices(
                    mask.data_ptr(), col_sz.data_ptr(), kv_indptr.data_ptr(), H, MB, NB, g, kv_len, num_pages,
                    kv_indices.numel(), kv_indices.data_ptr(), _lib.current_stream(dev)),
                "VariableBlockSparseAttentionWrapper.plan")

        qo_indptr_host = torch.zeros((H * MB + 1,), dtype=torch.int32)
        qo_indptr_host[1:] = torch.cumsum(row_host.flatten(), 0)
        self._active = None
        self._prefill.plan(
            qo_indptr_host, kv_indptr_host, kv_indices, torch.full((H * MB,), g, dtype=torch.int32, device=dev),
            num_qo_heads // num_kv_heads, 1, head_dim, g, causal=causal, pos_encoding_mode=pos_encoding_mode,
            sm_scale=sm_scale, logits_soft_cap=logits_soft_cap, rope_scale=rope_scale, rope_theta=rope_theta,
            q_data_type=q_data_type, kv_data_type=kv_data_type, non_blocking=non_blocking,
            seq_lens=(kv_indptr_host[1:] - kv_indptr_host[:-1]) * g)
        self._active = self._prefill
        self._num_qo_heads, self._num_kv_heads, self._head_dim = num_qo_heads, num_kv_heads, head_dim
        self._gqa_group_size = num_qo_heads // num_kv_heads
        self._qo_len, self._kv_len, self._page_size = qo_len, kv_len, g

    def forward(
        self,
        q: torch.Tensor,
        k: torch.Tensor,
        v: torch.Tensor,
        pos_encoding_mode: str = "NONE",
        use_fp16_qk_reduction: bool = False,
        logits_soft_cap: Optional[float] = None,
        sm_scale: Optional[float] = None,
        rope_scale: Optional[float] = None,
        rope_theta: Optional[float] = None,
    ) -> torch.Tensor:
        r"""Warning: This method is deprecated, please use :meth:`run` instead."""
        self._set_forward_options(pos_encoding_mode, logits_soft_cap, sm_scale, rope_scale, rope_theta)
        return self.run(q, k, v)

    def run(
        self,
        q: torch.Tensor,
        k: torch.Tensor,
        v: torch.Tensor,
        out: Optional[torch.Tensor] = None,
        lse: Optional[torch.Tensor] = None,
        return_lse: bool = False,
        enable_pdl: Optional[bool] = None,
    ) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        r"""Compute block-sparse attention between Q/K/V tensors (all heads-first).

        q : ``(num_qo_heads, qo_len, head_dim)``; k, v : ``(num_kv_heads, kv_len, head_dim)``, read in place when
        contiguous.
        out : ``(num_qo_heads, qo_len, head_dim)`` of q's dtype; lse : float32 ``(num_qo_heads, qo_len)``; both
            optional.  With ``num_qo_heads == num_kv_heads`` q is read and a contiguous ``out`` / ``lse`` written in
            place; with a larger group q is regrouped to ``(num_kv_heads * qo_len, group, head_dim)`` and the results
            regrouped back, one copy each way (as in the reference).
        enable_pdl : accepted and unused.
        Returns the output, and with ``return_lse`` the base-2 logsumexp ``(num_qo_heads, qo_len)``.
        (ref: flashinfer/sparse.py:1099-1269)
        """
        w = self._planned()
        for t, name in ((q, "q"), (k, "k"), (v, "v")):
            _lib.require_gpu_tensor(t, name)
        Hq, Hkv, D, group = self._num_qo_heads, self._num_kv_heads, self._head_dim, self._gqa_group_size
        if tuple(q.shape) != (Hq, self._qo_len, D):
            raise ValueError(f"q must have shape ({Hq}, {self._qo_len}, {D}), got {tuple(q.shape)}")
        kv_shape = (Hkv, self._kv_len, D)
        if tuple(k.shape) != kv_shape or tuple(v.shape) != kv_shape:
            raise ValueError(f"k and v must have shape {kv_shape}, got {tuple(k.shape)} / {tuple(v.shape)}")
        if out is not None and (tuple(out.shape) != tuple(q.shape) or out.dtype != q.dtype or out.device != q.device):
            raise ValueError(f"out must have shape {tuple(q.shape)} and dtype {q.dtype} on {q.device}")
        if lse is not None and (tuple(lse.shape) != (Hq, self._qo_len) or lse.dtype != torch.float32
                                or lse.device != q.device):
            raise ValueError(f"lse must be float32 with shape ({Hq}, {self._qo_len}) on {q.device}")
        rows = Hkv * self._qo_len
        kv = (k.reshape(-1, self._page_size, 1, D), v.reshape(-1, self._page_size, 1, D))
        if group == 1:
            # heads-first rows are the kernel's rows already
            direct_out = out is not None and out.is_contiguous()
            direct_lse = return_lse and lse is not None and lse.is_contiguous()
            res = w.run(q.reshape(rows, 1, D), kv, out=out.view(rows, 1, D) if direct_out else None,
                        lse=lse.view(rows, 1) if direct_lse else None, return_lse=return_lse)
            o, s = res if return_lse else (res, None)
            o, s = o.view(Hq, self._qo_len, D), None if s is None else s.view(Hq, self._qo_len)
        else:
            q = q.reshape(Hkv, group, self._qo_len, D).permute(0, 2, 1, 3).reshape(rows, group, D)
            res = w.run(q, kv, return_lse=return_lse)
            o, s = res if return_lse else (res, None)
            o = o.view(Hkv, self._qo_len, group, D).permute(0, 2, 1, 3).reshape(Hq, self._qo_len, D)
            if s is not None:
                s = s.view(Hkv, self._qo_len, group).permute(0, 2, 1).reshape(Hq, self._qo_len)
        if out is not None and o.data_ptr() != out.data_ptr():
            o = out.copy_(o)
        elif out is not None:
            o = out
        if s is not None and lse is not None:
            s = lse if s.data_ptr() == lse.data_ptr() else lse.copy_(s)
        return (o, s) if return_lse else o
