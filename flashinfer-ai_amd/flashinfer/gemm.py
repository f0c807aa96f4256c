"""fp8 groupwise-scaled GEMM operators (``gemm_fp8_nt_groupwise``, ``group_gemm_fp8_nt_groupwise``), the grouped
GEMM with MXFP8 activations and MXFP4 weights (``group_gemm_mxfp8_mxfp4_nt_groupwise``) and the dense MXFP4 x MXFP4
matmul (``mm_fp4`` in its ``use_nvfp4=False`` mode).

API of the reference's ``flashinfer/gemm.py`` (:2321-2484, :2657-2811, :2814-2949, :2012-2160); the kernels are
csrc/gemm.hip (MFMA fp8, two-level accumulation per 128-wide K block), csrc/gemm_mxfp4.hip and csrc/mm_fp4.hip
(block-scaled MFMA, the E8M0 scale bytes ride the instruction's scale operands).  NVIDIA-only knobs (``mma_sm``, ``backend``, tile shapes, ``swap_ab``)
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
