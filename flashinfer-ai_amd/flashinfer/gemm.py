"""fp8 groupwise-scaled GEMM operators (``gemm_fp8_nt_groupwise``, ``group_gemm_fp8_nt_groupwise``), the grouped
GEMM with MXFP8 activations and MXFP4 weights (``group_gemm_mxfp8_mxfp4_nt_groupwise``) and the dense MXFP4 x MXFP4
matmul (``mm_fp4`` in its ``use_nvfp4=False`` mode), the masked batched fp8 GEMM of expert-parallel decode
(``batch_deepgemm_fp8_nt_groupwise``), the contiguous-layout grouped fp8 GEMM of expert-parallel prefill
(``group_deepgemm_fp8_nt_groupwise``, on csrc/gemm_contig.hip: one group per 128-row block, named by a per-row index
on the device), the f16 / bf16 segment GEMM of multi-LoRA serving (``SegmentGEMMWrapper``), and
the batched fp8 matmul with one scale per tensor (``bmm_fp8``, on csrc/bmm_fp8.hip: the weight stream of
csrc/gemm_masked.hip with one accumulator chain, k / n / m tails and a form whose waves split k).

API of the reference's ``flashinfer/gemm.py`` (:2321-2484, :2657-2811, :2814-2949, :2012-2160, :3121-3256, :1300-1553,
:2227-2318); the kernels are
csrc/gemm.hip (MFMA fp8, two-level accumulation per 128-wide K block), csrc/gemm_mxfp4.hip and csrc/mm_fp4.hip
(block-scaled MFMA, the E8M0 scale bytes ride the instruction's scale operands) and csrc/gemm_masked.hip (weight
streaming, tile list built on the device) and csrc/segment_gemm.hip (skinny grouped GEMM in two forms, segment records
built on the device).  NVIDIA-only knobs (``mma_sm``, ``backend``, tile shapes, ``swap_ab``)
are accepted and ignored.
"""
from __future__ import annotations

import ctypes as C
from typing import Literal, Optional, Tuple

import torch

from . import _lib

_FP8 = (torch.float8_e4m3fn, torch.float8_e5m2)


def _validate_fp8_output_dtype(dtype: torch.dtype) -> None:
    if dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"Unsupported output dtype: {dtype}. Only torch.bfloat16 and torch.float16 are supported.")


def bmm_fp8(
    A: torch.Tensor,
    B: torch.Tensor,
    A_scale: torch.Tensor,
    B_scale: torch.Tensor,
    dtype: torch.dtype,
    out: Optional[torch.Tensor] = None,
    backend: Literal["cudnn", "cublas", "cutlass", "auto"] = "cublas",
) -> torch.Tensor:
    r"""Batched fp8 matmul with one scale per tensor (ref: flashinfer/gemm.py:2227-2318)::

        out[b, i, j] = dtype(A_scale * B_scale * sum_k A[b, i, k] * B[b, k, j])

    f32 accumulation over the whole of ``k``, one multiply by ``A_scale * B_scale`` in f32, one rounding to nearest.  The
    kernel is csrc/bmm_fp8.hip: the weights stream from global memory into the fp8 MFMA, in row tiles of 16 to 128 tokens;
    for few tokens and few tiles (a decode-time linear layer) the four waves of a workgroup split ``k`` between them.  It
    serves a dense prefill-size GEMM (``m`` in the thousands) correctly but is not tuned for it: a 256-wide MFMA-bound
    tile for that regime is not provided.

    A : ``(b, m, k)`` float8_e4m3fn or float8_e5m2, contiguous.
    B : ``(b, k, n)`` float8_e4m3fn or float8_e5m2, COLUMN-major: ``B.transpose(-2, -1)`` must be contiguous, the storage
        is ``(b, n, k)``.  There is no silent copy of a weight tensor: anything else raises ValueError.  ``A`` and ``B`` both
        float8_e5m2 raises ValueError (the reference's cuBLAS path has no such product).
    A_scale, B_scale : float32 tensors of exactly one element, of any shape, on the device.  The kernel reads them, the
        host never does: no synchronisation, so the call can be captured into a graph, and a replay uses what the scale
        tensors hold then.
    dtype : torch.bfloat16 or torch.float16.
    out : optional contiguous ``(b, m, n)`` tensor of ``dtype``; it is returned.
    backend : one of the reference's names, checked and then ignored.
    ``k % 16 == 0``, ``k > 0`` and ``n % 8 == 0``; any ``m >= 0`` and ``b >= 0``.  Nothing needs to be a multiple of 128.

    Examples
    --------
    >>> import torch
    >>> import torch.nn.functional as F
    >>> import flashinfer
    >>> def to_float8(x, dtype=torch.float8_e4m3fn):
    ...     finfo = torch.finfo(dtype)
    ...     min_val, max_val = x.aminmax()
    ...     amax = torch.maximum(min_val.abs(), max_val.abs()).clamp(min=1e-12)
    ...     scale = finfo.max / amax
    ...     x_scl_sat = (x * scale).clamp(min=finfo.min, max=finfo.max)
    ...     return x_scl_sat.to(dtype), scale.float().reciprocal()
    >>>
    >>> input = torch.randn([16, 48, 64], device="cuda", dtype=torch.bfloat16)
    >>> input_fp8, input_inv_s = to_float8(input, dtype=torch.float8_e4m3fn)
    >>> # column major weight
    >>> weight = torch.randn([16, 80, 64], device="cuda", dtype=torch.bfloat16).transpose(-2, -1)
    >>> weight_fp8, weight_inv_s = to_float8(weight, dtype=torch.float8_e4m3fn)
    >>> out = flashinfer.bmm_fp8(input_fp8, weight_fp8, input_inv_s, weight_inv_s, torch.bfloat16)
    >>> out.shape
    torch.Size([16, 48, 80])
    >>> out.dtype
    torch.bfloat16
    """
    _validate_fp8_output_dtype(dtype)
    if backend not in ("cudnn", "cublas", "cutlass", "auto"):
        raise ValueError(f"Unsupported backend: {backend}")
    if A.dtype not in _FP8 or B.dtype not in _FP8:
        raise ValueError(f"A and B must be float8_e4m3fn or float8_e5m2, got {A.dtype} and {B.dtype}")
    if A.dtype == torch.float8_e5m2 and B.dtype == torch.float8_e5m2:
        raise ValueError("A and B are both float8_e5m2: at least one operand must be float8_e4m3fn")
    if A.ndim != 3 or B.ndim != 3:
        raise ValueError(f"A must be (b, m, k) and B (b, k, n), got A.shape = {tuple(A.shape)}, B.shape = {tuple(B.shape)}")
    batch, m, k = A.shape
    n = B.shape[2]
    if B.shape[0] != batch or B.shape[1] != k:
        raise ValueError(f"Shape mismatch. A.shape = {tuple(A.shape)}, B.shape = {tuple(B.shape)}")
    if k == 0 or k % 16 != 0:
        raise ValueError(f"k = {k} must be a positive multiple of 16")
    if n % 8 != 0:
        raise ValueError(f"n = {n} must be a multiple of 8")
    if not A.is_contiguous():
        raise ValueError(f"A must be contiguous, got strides {A.stride()}")
    if not B.transpose(-2, -1).is_contiguous():
        raise ValueError(f"B must be column-major (b, k, n): pass w.transpose(-2, -1) of the (b, n, k) weight; got strides "
                         f"{B.stride()} and there is no silent copy of a weight tensor")
    for t, name in ((A_scale, "A_scale"), (B_scale, "B_scale")):
        if t.dtype != torch.float32 or t.numel() != 1:
            raise ValueError(f"{name} must be a float32 tensor of one element, got {t.dtype} with {t.numel()} elements")
    tensors = ((A, "A"), (B, "B"), (A_scale, "A_scale"), (B_scale, "B_scale"))
    if out is not None:
        tensors += ((out, "out"),)
        if tuple(out.shape) != (batch, m, n):
            raise ValueError(f"Output shape mismatch. Expected {(batch, m, n)}, got {tuple(out.shape)}.")
        if out.dtype != dtype:
            raise ValueError(f"Output dtype mismatch. Expected {dtype}, got {out.dtype}.")
        if not out.is_contiguous():
            raise ValueError("out must be contiguous")
    for t, name in tensors:
        _lib.require_gpu_tensor(t, name)
    for t, name in tensors:
        if t.device != A.device:
            raise ValueError(f"{name} is on {t.device}, A on {A.device}: they must share one device")
    if out is None:
        out = torch.empty((batch, m, n), device=A.device, dtype=dtype)
    if batch == 0 or m == 0 or n == 0:
        return out
    p = _lib.fi_bmm_fp8_params_t(
        a=A.data_ptr(), b=B.data_ptr(), a_scale=A_scale.data_ptr(), b_scale=B_scale.data_ptr(), d=out.data_ptr(),
        a_stride_b=m * k, b_stride_b=n * k, d_stride_b=m * n, batch=batch, m=m, n=n, k=k,
        a_dtype=_lib.fi_dtype(A.dtype), b_dtype=_lib.fi_dtype(B.dtype), d_dtype=_lib.fi_dtype(dtype))
    with torch.cuda.device(A.device):
        _lib.check(_lib.lib().fi_bmm_fp8(C.byref(p), _lib.current_stream(A.device)), "bmm_fp8")
    return out


def gemm_fp8_nt_groupwise(
    a: torch.Tensor,
    b: torch.Tensor,
    a_scale: torch.Tensor,
    b_scale: torch.Tensor,
    scale_major_mode: Optional[Literal["MN", "K"]] = None,
    mma_sm: int = 1,
    scale_granularity_mnk: Tuple[int, int, int] = (1, 128, 128),
    out: Optional[torch.Tensor] = None,
    out_dtype: Optional[torch.dtype] = None,
    backend: Literal["cutlass", "trtllm"] = "cutlass",
) -> torch.Tensor:
    r"""``out = (a * a_scale) @ (b * b_scale)^T`` with fp8 inputs and groupwise scales.

    a : ``(m, k)`` fp8 row-major; b : ``(n, k)`` fp8.
    a_scale : ``(ceil(m / gm), k // 128)`` if ``scale_major_mode == "K"`` else ``(k // 128, ceil(m / gm))``: row
        ``r`` of ``a`` uses scale row ``r // gm``.
    b_scale : ``(n // 128, k // 128)`` if ``"K"`` else ``(k // 128, n // 128)``.
    scale_granularity_mnk : ``(gm, 128, 128)`` with ``gm`` 1 or 128.
    out / out_dtype : ``(m, n)`` bf16 (default) or fp16.
    """
    for t, name in ((a, "a"), (b, "b"), (a_scale, "a_scale"), (b_scale, "b_scale")):
        _lib.require_gpu_tensor(t, name)
    if a.ndim != 2 or b.ndim != 2:
        raise ValueError(f"Shape mismatch. a.shape = {a.shape}, b.shape = {b.shape}")
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"Shape mismatch. a.shape[1] = {a.shape[1]}, b.shape[1] = {b.shape[1]}")
    if a.dtype not in _FP8 or b.dtype not in _FP8:
        raise ValueError("a and b must be float8_e4m3fn or float8_e5m2")
    if scale_major_mode is None:
        scale_major_mode = "MN"
    if scale_major_mode not in ("MN", "K"):
        raise ValueError(f"Invalid scale_major_mode {scale_major_mode}")
    if out is None:
        out_dtype = out_dtype or torch.bfloat16
    else:
        out_dtype = out.dtype
    _validate_fp8_output_dtype(out_dtype)
    m, k = a.shape
    n = b.shape[0]
    if out is None:
        out = torch.empty(m, n, device=a.device, dtype=out_dtype)
    elif out.shape != (m, n) or not out.is_contiguous():
        raise ValueError("out must be a contiguous (m, n) tensor")
    a, b = a.contiguous(), b.contiguous()
    a_scale = a_scale.to(torch.float32).contiguous()
    b_scale = b_scale.to(torch.float32).contiguous()
    gm, gn, gk = scale_granularity_mnk
    with torch.cuda.device(a.device):
        _lib.check(
            _lib.lib().fi_gemm_fp8_nt_groupwise(
                a.data_ptr(), b.data_ptr(), a_scale.data_ptr(), b_scale.data_ptr(), out.data_ptr(), m, n, k,
                gm, gn, gk, int(scale_major_mode == "K"), _lib.fi_dtype(a.dtype), _lib.fi_dtype(b.dtype),
                _lib.fi_dtype(out_dtype), _lib.current_stream(a.device),
            ),
            "gemm_fp8_nt_groupwise",
        )
    return out


def group_gemm_fp8_nt_groupwise(
    a: torch.Tensor,  # (cum_m, k)
    b: torch.Tensor,  # (batch_size, n, k)
    a_scale: torch.Tensor,  # (k // block_size, cum_m)
    b_scale: torch.Tensor,  # (batch_size, k // block_size, n // block_size)
    m_indptr: torch.Tensor,  # (batch_size + 1, )
    scale_granularity_mnk: Tuple[int, int, int] = (1, 128, 128),
    scale_major_mode: Literal["MN", "K"] = "MN",
    mma_sm: int = 1,
    out: Optional[torch.Tensor] = None,  # (cum_m, n)
    out_dtype: Optional[torch.dtype] = None,
) -> torch.Tensor:
    r"""Grouped GEMM with fp8 inputs and groupwise scales: rows ``m_indptr[g]:m_indptr[g+1]`` of ``a``
    are multiplied with ``b[g]^T``.

    a : ``(cum_m, k)`` fp8; b : ``(batch_size, n, k)`` fp8.
    a_scale : float32, ``(ceil(cum_m / gm), k // 128)`` if ``"K"`` else ``(k // 128, ceil(cum_m / gm))``: ``cum_m``
        scale rows with ``gm == 1``, ``ceil(cum_m / 128)`` with ``gm == 128``.  Group ``g``'s rows use the scale rows
        from ``m_indptr[g] // gm`` on, blocked from the group's first row: row ``r`` of the group uses scale row
        ``m_indptr[g] // gm + r // gm`` (the reference offsets the scale pointer per group by ``sf_m_offset``,
        include/flashinfer/gemm/group_gemm_fp8_groupwise_sm100.cuh:52-69).
    b_scale : ``(batch_size, n // 128, k // 128)`` if ``"K"`` else ``(batch_size, k // 128, n // 128)``.
    scale_granularity_mnk : ``(gm, 128, 128)`` with ``gm`` 1 or 128.
    m_indptr : ``(batch_size + 1,)`` int32, each entry a multiple of 4.
    out : ``(cum_m, n)`` bf16 (default) / fp16.
    """
    for t, name in ((a, "a"), (b, "b"), (a_scale, "a_scale"), (b_scale, "b_scale"), (m_indptr, "m_indptr")):
        _lib.require_gpu_tensor(t, name)
    assert a.dtype in _FP8
    assert b.dtype in _FP8
    assert a_scale.dtype == torch.float32
    assert b_scale.dtype == torch.float32
    assert m_indptr.dtype == torch.int32
    assert scale_major_mode in ["MN", "K"]
    assert mma_sm in [1, 2]
    if out is None:
        if out_dtype is None:
            out_dtype = torch.bfloat16
    else:
        if out_dtype is None:
            out_dtype = out.dtype
    _validate_fp8_output_dtype(out_dtype)
    num_groups = m_indptr.shape[0] - 1
    assert b.shape[0] == num_groups
    n = b.shape[1]
    k = b.shape[2]
    assert a.shape[1] == k
    assert n % 8 == 0
    assert k % 16 == 0
    out_shape = (a.shape[0], n)
    if out is None:
        out = torch.empty(out_shape, dtype=out_dtype, device=a.device)
    else:
        assert out.shape == out_shape
        assert out.dtype == out_dtype
        assert out.is_contiguous()
    a, b = a.contiguous(), b.contiguous()
    a_scale, b_scale, m_indptr = a_scale.contiguous(), b_scale.contiguous(), m_indptr.contiguous()
    gm, gn, gk = scale_granularity_mnk
    with torch.cuda.device(a.device):
        _lib.check(
            _lib.lib().fi_group_gemm_fp8_nt_groupwise(
                a.data_ptr(), b.data_ptr(), a_scale.data_ptr(), b_scale.data_ptr(), out.data_ptr(),
                m_indptr.data_ptr(), num_groups, a.shape[0], n, k, gm, gn, gk, int(scale_major_mode == "K"),
                _lib.fi_dtype(a.dtype), _lib.fi_dtype(b.dtype), _lib.fi_dtype(out_dtype),
                _lib.current_stream(a.device),
            ),
            "group_gemm_fp8_nt_groupwise",
        )
    return out


def _group_gemm_fp8_into(a: torch.Tensor, b: torch.Tensor, a_scale: torch.Tensor, b_scale: torch.Tensor,
                         out: torch.Tensor, m_indptr: torch.Tensor, scale_k_major: bool = True) -> None:
    """fi_group_gemm_fp8_nt_groupwise with (1, 128, 128) scales on checked tensors, into ``out``: no allocation, no
    dtype conversion, no copy -- every tensor is contiguous as it comes.  ``a`` ``(rows, k)`` and ``out`` ``(rows, n)`` may
    have more rows than ``m_indptr[-1]`` (the fused MoE layer with a local expert window): the kernels take their row
    tiles from the groups (csrc/gemm_common.h, group_of_tile), so those rows of ``a`` are never loaded and those of
    ``out`` never stored; ``a_scale`` must hold finite values for all ``rows`` (the power-of-two check reads them all)."""
    for t, name in ((a, "a"), (b, "b"), (a_scale, "a_scale"), (b_scale, "b_scale"), (out, "out"), (m_indptr, "m_indptr")):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if a_scale.dtype != torch.float32 or b_scale.dtype != torch.float32:
        raise ValueError("a_scale and b_scale must be float32")
    num_groups, n, k = b.shape
    with torch.cuda.device(a.device):
        _lib.check(
            _lib.lib().fi_group_gemm_fp8_nt_groupwise(
                a.data_ptr(), b.data_ptr(), a_scale.data_ptr(), b_scale.data_ptr(), out.data_ptr(),
                m_indptr.data_ptr(), num_groups, a.shape[0], n, k, 1, 128, 128, int(bool(scale_k_major)),
                _lib.fi_dtype(a.dtype), _lib.fi_dtype(b.dtype), _lib.fi_dtype(out.dtype),
                _lib.current_stream(a.device),
            ),
            "group_gemm_fp8_nt_groupwise",
        )


def _group_gemm_mxfp4_into(a: torch.Tensor, b: torch.Tensor, a_scale: torch.Tensor, b_scale: torch.Tensor,
                           out: torch.Tensor, m_indptr: torch.Tensor, n: int, k: int) -> None:
    """fi_group_gemm_mxfp8_mxfp4_nt_groupwise on checked tensors; the scale buffers' sizes go along and are checked on
    the host against (cum_m + 127 G) // 128 * 128 rows and n padded to 128, without reading m_indptr."""
    a, b = a.contiguous(), b.contiguous()
    a_scale, b_scale, m_indptr = a_scale.contiguous(), b_scale.contiguous(), m_indptr.contiguous()
    if not out.is_contiguous():
        raise ValueError("out must be contiguous")
    p = _lib.fi_group_gemm_mxfp4_params_t(
        a=a.data_ptr(), b=b.data_ptr(), a_scale=a_scale.data_ptr(), b_scale=b_scale.data_ptr(), d=out.data_ptr(),
        m_indptr=m_indptr.data_ptr(), a_scale_bytes=a_scale.numel(), b_scale_bytes=b_scale.numel(),
        num_groups=m_indptr.shape[0] - 1, cum_m=a.shape[0], n=n, k=k, a_dtype=_lib.fi_dtype(a.dtype),
        d_dtype=_lib.fi_dtype(out.dtype))
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().fi_group_gemm_mxfp8_mxfp4_nt_groupwise(C.byref(p), _lib.current_stream(a.device)),
                   "group_gemm_mxfp8_mxfp4_nt_groupwise")


def group_gemm_mxfp8_mxfp4_nt_groupwise(
    a: torch.Tensor,  # (cum_m, k)
    b: torch.Tensor,  # (batch_size, n, k // 2)
    a_scale: torch.Tensor,  # (cum_m_padded, k // 32)
    b_scale: torch.Tensor,  # (batch_size, n_padded, k // 32)
    m_indptr: torch.Tensor,  # (batch_size + 1, )
    mma_sm: int = 1,
    tile_m: int = 128,
    tile_n: int = 128,
    tile_k: int = 128,
    swap_ab: bool = True,
    out: Optional[torch.Tensor] = None,  # (cum_m, n)
    out_dtype: Optional[torch.dtype] = None,
) -> torch.Tensor:
    r"""Grouped GEMM with MXFP8 activations and MXFP4 weights (ref: flashinfer/gemm.py:2814-2945): rows
    ``m_indptr[g]:m_indptr[g+1]`` of ``a`` are multiplied with ``b[g]^T``; every 32 consecutive k elements of a row of
    either operand carry one E8M0 scale byte.  The kernel is csrc/gemm_mxfp4.hip (block-scaled MFMA, no dequantisation).

    a : ``(cum_m, k)`` float8_e4m3fn or float8_e5m2.
    b : ``(batch_size, n, k // 2)`` uint8, two e2m1 codes per byte, element ``2 i`` in the low nibble of byte ``i``.
    a_scale : uint8, ``((cum_m + 127 * batch_size) // 128 * 128, k // 32)``: the rows of group ``g`` start at scale row
        ``(m_indptr[g] + 127 g) // 128 * 128`` and are in the swizzled "128x4" layout from there
        (``flashinfer.fp8_quantization.mxfp8_quantize_grouped`` produces it).
    b_scale : uint8, ``(batch_size, ceil(n / 128) * 128, k // 32)``, every group swizzled on its own.
    m_indptr : ``(batch_size + 1,)`` int32 on the device; it is not read on the host.
    mma_sm, tile_m, tile_n, tile_k, swap_ab : the reference's NVIDIA tuning knobs; validated as there, then ignored.
    out : ``(cum_m, n)`` bf16 (default) / fp16; rows at or past ``m_indptr[-1]`` are not written.
    ``n % 8 == 0`` and ``k % 128 == 0``.
    """
    for t, name in ((a, "a"), (b, "b"), (a_scale, "a_scale"), (b_scale, "b_scale"), (m_indptr, "m_indptr")):
        _lib.require_gpu_tensor(t, name)
    assert a.dtype in [torch.float8_e4m3fn, torch.float8_e5m2]
    assert b.dtype == torch.uint8
    assert a_scale.dtype == torch.uint8
    assert b_scale.dtype == torch.uint8
    assert m_indptr.dtype == torch.int32
    assert mma_sm in [1, 2]
    assert tile_m in [128]
    assert tile_n in [64, 128, 192, 256]
    assert tile_k in [128, 256]
    assert swap_ab in [True, False]
    if out is None:
        if out_dtype is None:
            out_dtype = torch.bfloat16
    else:
        if out_dtype is None:
            out_dtype = out.dtype
    assert out_dtype in [torch.bfloat16, torch.float16]
    num_groups = m_indptr.shape[0] - 1
    assert b.shape[0] == num_groups
    n = b.shape[1]
    k = b.shape[2] * 2  # two e2m1 codes per byte
    assert a.shape[1] == k
    assert n % 8 == 0
    assert k % 128 == 0
    out_shape = (a.shape[0], n)
    if out is None:
        out = torch.empty(out_shape, dtype=out_dtype, device=a.device)
    else:
        assert out.shape == out_shape
        assert out.dtype == out_dtype
    _group_gemm_mxfp4_into(a, b, a_scale, b_scale, out, m_indptr, n, k)
    return out


# the reference keeps the old name (gemm.py:2948-2949)
group_gemm_mxfp4_nt_groupwise = group_gemm_mxfp8_mxfp4_nt_groupwise

_FP4_BYTES = tuple(t for t in (torch.uint8, getattr(torch, "float4_e2m1fn_x2", None)) if t is not None)
_SF_BYTES = (torch.float8_e4m3fn, torch.uint8)


def _scale_bytes(t: torch.Tensor, name: str, transposed_ok: bool) -> torch.Tensor:
    """The storage of a swizzled scale tensor as flat uint8, without a copy."""
    if transposed_ok and t.ndim == 2 and t.stride(0) == 1 and t.T.is_contiguous():
        t = t.T  # the reference's sf.T: the storage is read in order
    elif transposed_ok and t.ndim != 1 or not t.is_contiguous():
        form = "the transposed view sf.T of mxfp4_quantize's scales (2-D, stride(0) == 1) or a flat tensor of its bytes" \
            if transposed_ok else "contiguous"
        raise ValueError(f"{name} must be {form}, got shape {tuple(t.shape)} with strides {t.stride()}")
    return t.view(torch.uint8).reshape(-1)


def mm_fp4(
    a: torch.Tensor,
    b: torch.Tensor,
    a_descale: torch.Tensor,
    b_descale: torch.Tensor,
    alpha: Optional[torch.Tensor] = None,
    out_dtype: torch.dtype = torch.bfloat16,
    out: Optional[torch.Tensor] = None,
    block_size: int = 16,
    use_8x4_sf_layout: bool = False,
    backend: Literal["cudnn", "trtllm", "cutlass"] = "cudnn",
    use_nvfp4: bool = True,
) -> torch.Tensor:
    r"""``out = alpha * dequant(a) @ dequant(b)`` with both operands MXFP4 (ref: flashinfer/gemm.py:2012-2160), f32
    accumulation, ``alpha`` multiplied in f32, one rounding to ``out_dtype``.  The kernels are csrc/mm_fp4.hip (block-scaled
    fp4 x fp4 MFMA; weight streaming for few rows, 128 x 128 LDS tiles for many).

    Only ``use_nvfp4=False, block_size=32, use_8x4_sf_layout=False`` runs.  The defaults select nvfp4 (16-element blocks,
    e4m3 scales, a global scale), which is not provided, so a bare call raises NotImplementedError; so does the 8x4 layout.

    a : ``(m, k / 2)`` uint8 (or float4_e2m1fn_x2) row-major: what ``mxfp4_quantize(x)`` returns.
    b : ``(k / 2, n)`` COLUMN-major: ``w_q.T`` of the ``(n, k / 2)`` tensor ``mxfp4_quantize(w)`` returns.  There is no silent
        copy of a weight matrix: a ``b`` whose ``.T`` is not contiguous raises ValueError.
    a_descale : the swizzled "128x4" bytes of the ``(m, k / 32)`` scales, uint8 or float8_e4m3fn read as bytes, contiguous, in
        any shape with at least ``ceil(m / 128) * 128 * k / 32`` bytes.
    b_descale : the same for ``(n, k / 32)``, as the transposed view ``sf.T`` of what ``mxfp4_quantize(w)`` returns (2-D with
        ``stride(0) == 1``) or as a 1-D tensor of the bytes.
    alpha : None or a float32 tensor of one element on the device; the kernel reads it, the host never does.
    out_dtype / out : bf16 or f16; ``out``, if given, is contiguous ``(m, n)`` of ``out_dtype`` and is returned.
    backend : the reference's names, accepted and ignored.
    ``k % 128 == 0`` and ``n % 8 == 0``; any ``m >= 0``.  No host read of a device value, no synchronisation: the call can be
    captured into a graph.
    """
    if a.ndim != 2 or b.ndim != 2:
        raise ValueError(f"mm_fp4 accepts 2d tensors, got {a.shape} and {b.shape}")
    if a.shape[1] != b.shape[0]:
        raise ValueError(f"K dimension mismatch in mm_fp4. got a.shape[1] = {a.shape[1]}, b.shape[0] = {b.shape[0]}")
    if a.dtype not in _FP4_BYTES or b.dtype not in _FP4_BYTES:
        raise ValueError(f"a and b must have float4_e2m1fn_x2 packed into uint8. Got {a.dtype} and {b.dtype}.")
    if a_descale.dtype not in _SF_BYTES or b_descale.dtype not in _SF_BYTES:
        raise ValueError(f"a_descale and b_descale must have float8_e4m3fnx2 packed into uint8. "
                         f"Got {a_descale.dtype} and {b_descale.dtype}.")
    if alpha is not None and alpha.dtype != torch.float:
        raise ValueError(f"alpha must be a float tensor, got {alpha.dtype}")
    if alpha is not None and alpha.numel() != 1:
        raise ValueError(f"alpha must be a scalar, got {alpha.numel()}")
    if out_dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"Unsupported output dtype: {out_dtype}. "
                         f"Only torch.bfloat16 and torch.float16 are supported for FP4 GEMM operations.")
    if use_nvfp4 and block_size != 16:
        raise ValueError("nvfp4 only supports block_size = 16.")
    if not use_nvfp4 and block_size != 32:
        raise ValueError("mxfp4 supports block_size = 32.")
    if backend not in ("cudnn", "trtllm", "cutlass"):
        raise ValueError(f"Invalid backend {backend!r}: expected 'cudnn', 'trtllm' or 'cutlass'")
    if use_nvfp4:
        raise NotImplementedError(
            "nvfp4 (block_size 16, e4m3 scales, a global scale) is not provided: only MXFP4, use_nvfp4=False with "
            "block_size=32, runs on this hardware")
    if use_8x4_sf_layout:
        raise NotImplementedError("the 8x4 layout of the scales is not provided: only 128x4")

    m, n, k = a.shape[0], b.shape[1], a.shape[1] * 2
    if k == 0 or k % 128 != 0:
        raise NotImplementedError(f"k = {k} (a.shape[1] * 2) must be a positive multiple of 128: pad a and b with zero codes")
    if n % 8 != 0:
        raise NotImplementedError(f"n = {n} (b.shape[1]) must be a multiple of 8: pad b with rows of zero codes")
    if not a.is_contiguous():
        raise ValueError(f"a must be row-major contiguous, got strides {a.stride()}")
    if not b.T.is_contiguous():
        raise ValueError(f"b must be column-major (k / 2, n): pass w_q.T of the (n, k / 2) quantised weight; got strides "
                         f"{b.stride()} and there is no silent copy of a weight matrix")
    sa = _scale_bytes(a_descale, "a_descale", False)
    sb = _scale_bytes(b_descale, "b_descale", True)
    if out is not None:
        if tuple(out.shape) != (m, n):
            raise ValueError(f"Output shape mismatch. Expected {(m, n)}, got {tuple(out.shape)}.")
        if out.dtype != out_dtype:
            raise ValueError(f"Output dtype mismatch. Expected {out_dtype}, got {out.dtype}.")
        if out.device != a.device:
            raise ValueError(f"Output device mismatch. Expected {a.device}, got {out.device}.")
        if not out.is_contiguous():
            raise ValueError("out must be contiguous")
    tensors = [(a, "a"), (b, "b"), (a_descale, "a_descale"), (b_descale, "b_descale")]
    for t, name in tensors + ([(alpha, "alpha")] if alpha is not None else []):
        _lib.require_gpu_tensor(t, name)
    if out is None:
        out = torch.empty((m, n), device=a.device, dtype=out_dtype)
    if m == 0 or n == 0:
        return out
    p = _lib.fi_mm_mxfp4_params_t(
        a=a.data_ptr(), b=b.data_ptr(), a_scale=sa.data_ptr(), b_scale=sb.data_ptr(), alpha=_lib.ptr(alpha),
        d=out.data_ptr(), a_scale_bytes=sa.numel(), b_scale_bytes=sb.numel(), m=m, n=n, k=k,
        d_dtype=_lib.fi_dtype(out_dtype))
    fi_mm_mxfp4 = _lib.lib().fi_mm_mxfp4
    with torch.cuda.device(a.device):
        _lib.check(fi_mm_mxfp4(C.byref(p), _lib.current_stream(a.device)), "mm_fp4")
    return out


def batch_deepgemm_fp8_nt_groupwise(
    a: torch.Tensor,  # (batch_size, m, k)
    b: torch.Tensor,  # (batch_size, n, k)
    a_scale: torch.Tensor,  # (batch_size, m, k // block_size)
    b_scale: torch.Tensor,  # (batch_size, n // block_size, k // block_size)
    masked_m: torch.Tensor,  # (batch_size, )
    expected_m: int,
    scale_granularity_mnk: Tuple[int, int, int] = (1, 128, 128),
    out: Optional[torch.Tensor] = None,  # (batch_size, m, n)
    out_dtype: Optional[torch.dtype] = None,
) -> torch.Tensor:
    r"""Masked batched fp8 GEMM with groupwise scales, the layout of a low-latency expert-parallel dispatch (ref:
    flashinfer/gemm.py:3121-3256): every expert ``e`` owns ``m`` rows of ``a`` and ``out`` and ``masked_m[e]`` says how
    many leading rows are real.  With ``r = min(masked_m[e], m)``::

        out[e, :r] = (a[e, :r] * a_scale[e, :r] per 128-block) @ (b[e] * b_scale[e] per block).T

    f32 accumulation, every 128-wide k block's product scaled before it is added, one rounding.  The kernel is
    csrc/gemm_masked.hip (weight streaming, row tiles of 16 to 128 tokens, its tile list built from ``masked_m`` on the
    device).

    a : ``(E, m, k)`` float8_e4m3fn; rows ``r .. m - 1`` of ``a[e]`` and ``a_scale[e]`` are not read.
    b : ``(E, n, k)`` float8_e4m3fn.
    a_scale : ``(E, m, k // 128)`` float32; b_scale : ``(E, n // 128, k // 128)`` float32.
    masked_m : ``(E,)`` int32 on the device; the host never reads it, so the call can be captured into a graph and a
        replay follows what ``masked_m`` holds then.
    expected_m : a host-side hint (>= 1) for the rows per expert; it picks the row-tile height and never the result.
    scale_granularity_mnk : only ``(1, 128, 128)``.
    out / out_dtype : ``(E, m, n)`` bf16 (default) or fp16; rows ``r .. m - 1`` of ``out[e]`` keep what they held.
    ``n % 128 == 0``, ``k % 128 == 0``, ``E <= 1024``; every tensor contiguous.
    """
    tensors = ((a, "a"), (b, "b"), (a_scale, "a_scale"), (b_scale, "b_scale"), (masked_m, "masked_m"))
    if tuple(scale_granularity_mnk) != (1, 128, 128):
        raise NotImplementedError(f"scale_granularity_mnk = {tuple(scale_granularity_mnk)}: only (1, 128, 128) is provided")
    if a.dtype == torch.float8_e5m2 or b.dtype == torch.float8_e5m2:
        raise NotImplementedError("a / b in float8_e5m2 are not provided: only float8_e4m3fn")
    if a.dtype != torch.float8_e4m3fn or b.dtype != torch.float8_e4m3fn:
        raise ValueError(f"a and b must be float8_e4m3fn, got {a.dtype} and {b.dtype}")
    if a.ndim != 3 or b.ndim != 3:
        raise ValueError(f"a must be (E, m, k) and b (E, n, k), got a.shape = {tuple(a.shape)}, b.shape = {tuple(b.shape)}")
    num_experts, m, k = a.shape
    n = b.shape[1]
    if b.shape[0] != num_experts or b.shape[2] != k:
        raise ValueError(f"Shape mismatch. a.shape = {tuple(a.shape)}, b.shape = {tuple(b.shape)}")
    if n % 128 != 0 or k % 128 != 0:
        raise ValueError(f"n = {n} and k = {k} must be multiples of 128")
    if a_scale.dtype != torch.float32 or b_scale.dtype != torch.float32:
        raise ValueError(f"a_scale and b_scale must be float32, got {a_scale.dtype} and {b_scale.dtype}")
    if tuple(a_scale.shape) != (num_experts, m, k // 128):
        raise ValueError(f"a_scale must be {(num_experts, m, k // 128)}, got {tuple(a_scale.shape)}")
    if tuple(b_scale.shape) != (num_experts, n // 128, k // 128):
        raise ValueError(f"b_scale must be {(num_experts, n // 128, k // 128)}, got {tuple(b_scale.shape)}")
    if masked_m.dtype != torch.int32 or tuple(masked_m.shape) != (num_experts,):
        raise ValueError(f"masked_m must be int32 of shape {(num_experts,)}, got {masked_m.dtype} {tuple(masked_m.shape)}")
    if int(expected_m) < 1:
        raise ValueError(f"expected_m = {expected_m} must be at least 1")
    if out is None:
        out_dtype = out_dtype or torch.bfloat16
    else:
        if out_dtype is not None and out_dtype != out.dtype:
            raise ValueError(f"Output dtype mismatch. Expected {out_dtype}, got {out.dtype}.")
        out_dtype = out.dtype
        tensors += ((out, "out"),)
        if tuple(out.shape) != (num_experts, m, n):
            raise ValueError(f"out must be {(num_experts, m, n)}, got {tuple(out.shape)}")
    _validate_fp8_output_dtype(out_dtype)
    for t, name in tensors:
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous, got strides {t.stride()}")
    for t, name in tensors:
        _lib.require_gpu_tensor(t, name)
    if out is None:
        out = torch.empty((num_experts, m, n), device=a.device, dtype=out_dtype)
    p = _lib.fi_batch_gemm_fp8_nt_masked_params_t(
        a=a.data_ptr(), b=b.data_ptr(), a_scale=a_scale.data_ptr(), b_scale=b_scale.data_ptr(), d=out.data_ptr(),
        masked_m=masked_m.data_ptr(), a_stride_e=m * k, b_stride_e=n * k, d_stride_e=m * n, num_experts=num_experts,
        m=m, n=n, k=k, expected_m=int(expected_m), d_dtype=_lib.fi_dtype(out_dtype))
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().fi_batch_gemm_fp8_nt_masked(C.byref(p), _lib.current_stream(a.device)),
                   "batch_deepgemm_fp8_nt_groupwise")
    return out


def group_deepgemm_fp8_nt_groupwise(
    a: torch.Tensor,  # (m, k)
    b: torch.Tensor,  # (batch_size, n, k)
    a_scale: torch.Tensor,  # (m, k // block_size)
    b_scale: torch.Tensor,  # (batch_size, n // block_size, k // block_size)
    m_indices: torch.Tensor,  # (m, )
    scale_granularity_mnk: Tuple[int, int, int] = (1, 128, 128),
    out: Optional[torch.Tensor] = None,  # (m, n)
    out_dtype: Optional[torch.dtype] = None,
) -> torch.Tensor:
    r"""Grouped fp8 GEMM with groupwise scales in the contiguous layout of a normal-mode expert-parallel dispatch (ref:
    flashinfer/gemm.py:2991-3118): row ``r`` of ``a`` belongs to group ``m_indices[r]`` and every group's segment is
    padded to a multiple of 128 rows, so block ``i`` (rows ``128 i .. 128 i + 127``, the last one possibly short) has one
    group ``g = m_indices[128 i]``.  Segments may come in any order and a group may own several of them.  For the rows
    ``r`` of a block with ``0 <= g < G`` whose own index is not negative::

        out[r] = (a[r] * a_scale[r] per 128-block) @ (b[g] * b_scale[g] per block).T

    f32 accumulation, every 128-wide k block's product scaled before it is added, one rounding.  A block whose ``g`` is
    negative or ``>= G`` is dead: nothing is loaded for it and nothing stored.  Rows of a live block with a negative index
    are tail padding: their ``a`` / ``a_scale`` are not read and their ``out`` rows keep what they held.  A non-negative
    index that differs from its block's first one is a caller error; the block's ``g`` is used.  The kernel is
    csrc/gemm_contig.hip (128 x 256 tiles on a persistent grid, the group of a tile one scalar load).

    a : ``(m, k)`` float8_e4m3fn; b : ``(G, n, k)`` float8_e4m3fn.
    a_scale : ``(m, k // 128)`` float32; b_scale : ``(G, n // 128, k // 128)`` float32.
    m_indices : ``(m,)`` int32 on the device; the host never reads it, so the call can be captured into a graph and a
        replay follows what ``m_indices`` holds then.
    scale_granularity_mnk : only ``(1, 128, 128)``.
    out / out_dtype : ``(m, n)`` bf16 (default) or fp16.
    ``n % 128 == 0``, ``k % 128 == 0``, any ``m >= 0``; every tensor contiguous.
    """
    tensors = ((a, "a"), (b, "b"), (a_scale, "a_scale"), (b_scale, "b_scale"), (m_indices, "m_indices"))
    if tuple(scale_granularity_mnk) != (1, 128, 128):
        raise NotImplementedError(f"scale_granularity_mnk = {tuple(scale_granularity_mnk)}: only (1, 128, 128) is provided")
    if a.dtype == torch.float8_e5m2 or b.dtype == torch.float8_e5m2:
        raise NotImplementedError("a / b in float8_e5m2 are not provided: only float8_e4m3fn")
    if a.dtype != torch.float8_e4m3fn or b.dtype != torch.float8_e4m3fn:
        raise ValueError(f"a and b must be float8_e4m3fn, got {a.dtype} and {b.dtype}")
    if a.ndim != 2 or b.ndim != 3:
        raise ValueError(f"a must be (m, k) and b (G, n, k), got a.shape = {tuple(a.shape)}, b.shape = {tuple(b.shape)}")
    m, k = a.shape
    num_groups, n = b.shape[0], b.shape[1]
    if b.shape[2] != k:
        raise ValueError(f"Shape mismatch. a.shape = {tuple(a.shape)}, b.shape = {tuple(b.shape)}")
    if n % 128 != 0 or k % 128 != 0 or k == 0:
        raise ValueError(f"n = {n} and k = {k} must be multiples of 128 (k a positive one)")
    if a_scale.dtype != torch.float32 or b_scale.dtype != torch.float32:
        raise ValueError(f"a_scale and b_scale must be float32, got {a_scale.dtype} and {b_scale.dtype}")
    if tuple(a_scale.shape) != (m, k // 128):
        raise ValueError(f"a_scale must be {(m, k // 128)}, got {tuple(a_scale.shape)}")
    if tuple(b_scale.shape) != (num_groups, n // 128, k // 128):
        raise ValueError(f"b_scale must be {(num_groups, n // 128, k // 128)}, got {tuple(b_scale.shape)}")
    if m_indices.dtype != torch.int32 or tuple(m_indices.shape) != (m,):
        raise ValueError(f"m_indices must be int32 of shape {(m,)}, got {m_indices.dtype} {tuple(m_indices.shape)}")
    if out is None:
        out_dtype = out_dtype or torch.bfloat16
    else:
        if out_dtype is not None and out_dtype != out.dtype:
            raise ValueError(f"Output dtype mismatch. Expected {out_dtype}, got {out.dtype}.")
        out_dtype = out.dtype
        tensors += ((out, "out"),)
        if tuple(out.shape) != (m, n):
            raise ValueError(f"out must be {(m, n)}, got {tuple(out.shape)}")
    _validate_fp8_output_dtype(out_dtype)
    for t, name in tensors:
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous, got strides {t.stride()}")
    if m == 0:  # nothing to launch, wherever the tensors live
        return out if out is not None else torch.empty((0, n), device=a.device, dtype=out_dtype)
    for t, name in tensors:
        _lib.require_gpu_tensor(t, name)
    if out is None:
        out = torch.empty((m, n), device=a.device, dtype=out_dtype)
    p = _lib.fi_group_gemm_fp8_nt_contiguous_params_t(
        a=a.data_ptr(), b=b.data_ptr(), a_scale=a_scale.data_ptr(), b_scale=b_scale.data_ptr(), d=out.data_ptr(),
        m_indices=m_indices.data_ptr(), num_groups=num_groups, m=m, n=n, k=k, d_dtype=_lib.fi_dtype(out_dtype))
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().fi_group_gemm_fp8_nt_contiguous(C.byref(p), _lib.current_stream(a.device)),
                   "group_deepgemm_fp8_nt_groupwise")
    return out


class SegmentGEMMWrapper:
    r"""Segment GEMM for multi-LoRA batches (ref: flashinfer/gemm.py:1300-1553): the rows of ``x`` are cut into
    ``batch_size`` consecutive segments and segment ``i`` is multiplied by its own weight::

        y[seg i] = x[seg i] @ W[weight_indices[i]]        (W[i] without weight_indices)

    in float16 or bfloat16 with f32 accumulation and one rounding.  The kernel is csrc/segment_gemm.hip: a long-k form
    for the shrink step (``d_in -> r``) and a wide-n form for the expand step (``r -> d_out``) and every other shape,
    chosen from ``(d_in, d_out)`` alone.

    >>> workspace_buffer = torch.empty(128 * 1024 * 1024, dtype=torch.int8, device="cuda")
    >>> segment_gemm = SegmentGEMMWrapper(workspace_buffer)
    >>> seg_lens = torch.tensor([1, 2, 3, 4], dtype=torch.int64)
    >>> x = torch.randn(10, 128, device="cuda", dtype=torch.float16)
    >>> weights = torch.randn(4, 256, 128, device="cuda", dtype=torch.float16)  # column major
    >>> y = segment_gemm.run(x, weights, 4, True, seg_lens=seg_lens)             # y[1:3] == x[1:3] @ weights[1].T
    """

    def __init__(self, float_workspace_buffer: torch.Tensor, backend: str = "auto") -> None:
        r"""``float_workspace_buffer`` is kept for the reference's signature; the kernels need only the 1 MiB int
        workspace allocated here on the same device (the segment records).  ``backend`` is accepted and ignored."""
        self._int_workspace_buffer = torch.empty((1024 * 1024,), dtype=torch.int8, device=float_workspace_buffer.device)
        self._float_workspace_buffer = float_workspace_buffer
        self.backend = backend

    def reset_workspace_buffer(self, float_workspace_buffer: torch.Tensor, int_workspace_buffer: torch.Tensor) -> None:
        self._float_workspace_buffer = float_workspace_buffer
        self._int_workspace_buffer = int_workspace_buffer

    def run(
        self,
        x: torch.Tensor,
        weights: torch.Tensor,
        batch_size: int,
        weight_column_major: bool,
        out: Optional[torch.Tensor] = None,
        seg_lens: Optional[torch.Tensor] = None,
        seg_indptr: Optional[torch.Tensor] = None,
        weight_indices: Optional[torch.Tensor] = None,
    ) -> torch.Tensor:
        r"""x : ``(rows, d_in)`` float16 / bfloat16, contiguous.
        weights : ``(num_weights, d_out, d_in)`` if ``weight_column_major`` else ``(num_weights, d_in, d_out)``, the dtype
            of ``x``, contiguous (no silent copy of a weight tensor).  Both layouts are read as they lie.
        batch_size : the number of segments.
        out : ``(rows, d_out)``, the dtype of ``x``; allocated with ``torch.empty`` when not given.
        seg_lens / seg_indptr : int64 ``(batch_size,)`` resp. ``(batch_size + 1,)``; one of them, ``seg_indptr`` wins.
        weight_indices : optional int64 ``(batch_size,)``.
        The three index tensors may live on the CPU: they are moved to ``x.device``, and that is the only copy -- nothing
        is read back, so a call with device tensors can be captured into a graph.

        ``d_in`` and ``d_out`` must be multiples of 8 (16-byte rows, as in the reference).  Rows of ``out`` that no
        segment covers (at or past ``seg_indptr[-1]``) are NOT written; the reference zero-fills them.  Segment bounds are
        clamped into ``[0, rows]``, a segment of negative length is empty, and a segment whose weight id is outside
        ``[0, num_weights)`` is skipped, its rows not written; none of this is reported."""
        if seg_lens is None and seg_indptr is None:
            raise ValueError("Either seg_lens or seg_indptr should be provided.")
        if x.dtype in _FP8:
            raise NotImplementedError("float8 x (the reference's sm90-only mode) is not provided: float16 / bfloat16 only")
        if x.dtype == torch.float32:
            raise NotImplementedError("float32 x is not provided: float16 / bfloat16 only")
        if x.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"x must be float16 or bfloat16, got {x.dtype}")
        if weights.dtype != x.dtype or (out is not None and out.dtype != x.dtype):
            raise ValueError(f"x, weights and out must share one dtype, got {x.dtype}, {weights.dtype}"
                             + (f" and {out.dtype}" if out is not None else ""))
        if x.ndim != 2 or weights.ndim != 3:
            raise ValueError(f"x must be (rows, d_in) and weights 3-D, got {tuple(x.shape)} and {tuple(weights.shape)}")
        rows, d_in = x.shape
        num_weights = weights.shape[0]
        w_in, d_out = (weights.shape[2], weights.shape[1]) if weight_column_major else (weights.shape[1], weights.shape[2])
        if w_in != d_in:
            raise ValueError(f"Shape mismatch. x.shape = {tuple(x.shape)}, weights.shape = {tuple(weights.shape)}, "
                             f"weight_column_major = {bool(weight_column_major)}")
        if d_in % 8 != 0 or d_out % 8 != 0:
            raise ValueError(f"d_in = {d_in} and d_out = {d_out} must be multiples of 8")
        if out is not None and tuple(out.shape) != (rows, d_out):
            raise ValueError(f"Output tensor shape mismatch, expected {(rows, d_out)}, got {tuple(out.shape)}")
        if not weights.is_contiguous():
            raise ValueError(f"weights must be contiguous (no silent copy of a weight tensor), got strides {weights.stride()}")
        if not x.is_contiguous() or (out is not None and not out.is_contiguous()):
            raise ValueError("x and out must be contiguous")
        batch_size = int(batch_size)
        for t, name, length in ((seg_indptr, "seg_indptr", batch_size + 1),
                                (seg_lens if seg_indptr is None else None, "seg_lens", batch_size),
                                (weight_indices, "weight_indices", batch_size)):
            if t is not None and tuple(t.shape) != (length,):
                raise ValueError(f"{name} must have shape ({length},) for batch_size = {batch_size}, got {tuple(t.shape)}")
        ws = self._int_workspace_buffer
        if _lib.nbytes(ws) < 16 + 16 * batch_size:
            raise ValueError(f"the int workspace ({_lib.nbytes(ws)} bytes) cannot hold {batch_size} segment records "
                             f"({16 + 16 * batch_size} bytes)")
        tensors = ((x, "x"), (weights, "weights"), (ws, "int_workspace_buffer")) + (((out, "out"),) if out is not None else ())
        for t, name in tensors:
            if t.device != x.device:
                raise ValueError(f"{name} is on {t.device}, x on {x.device}: they must share one device")
        for t, name in tensors:
            _lib.require_gpu_tensor(t, name)
        if out is None:
            out = torch.empty((rows, d_out), dtype=x.dtype, device=x.device)
        seg, widx = (seg_indptr if seg_indptr is not None else seg_lens), weight_indices
        seg = seg.to(device=x.device, dtype=torch.int64).contiguous()
        if widx is not None:
            widx = widx.to(device=x.device, dtype=torch.int64).contiguous()

        def i64(t):  # the header types these three as const int64_t*
            return None if t is None else C.cast(t.data_ptr(), C.POINTER(C.c_int64))

        p = _lib.fi_segment_gemm_params_t(
            x=x.data_ptr(), weights=weights.data_ptr(), y=out.data_ptr(),
            seg_lens=i64(seg if seg_indptr is None else None),
            seg_indptr=i64(seg if seg_indptr is not None else None), weight_indices=i64(widx),
            int_workspace=ws.data_ptr(), int_workspace_bytes=_lib.nbytes(ws), rows=rows, d_in=d_in, d_out=d_out,
            batch_size=batch_size, num_weights=num_weights, weight_column_major=int(bool(weight_column_major)),
            dtype=_lib.fi_dtype(x.dtype))
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().fi_segment_gemm(C.byref(p), _lib.current_stream(x.device)), "SegmentGEMMWrapper.run")
        return out

    forward = run
