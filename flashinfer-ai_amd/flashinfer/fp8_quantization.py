"""MXFP8 quantisation: ``mxfp8_quantize`` and ``mxfp8_dequantize_host`` of the reference's flashinfer/fp8_quantization.py
(:179-239), and ``mxfp8_quantize_grouped``, this project's own extension that writes the scales where the grouped
MXFP4 GEMM reads them.  The kernel is csrc/mxfp8_quantize.hip behind fi_mxfp8_quantize (include/fi_mi355.h).
``fp8_quantize_1x128``, also this project's own, makes DeepSeek's fp8 block-scale activations (one f32 scale per row and
128 columns) for ``trtllm_fp8_block_scale_moe``; its kernel is csrc/fp8_block_quantize.hip.

An MXFP8 tensor is e4m3 values plus one E8M0 byte (value ``2^(byte - 127)``) per 32 consecutive elements of a row.
The scale of a block is the smallest power of two ``2^e`` with ``448 * 2^e >= amax``; the compare is exact (the
reference's approximate reciprocal may give ``e + 1`` at ``amax == 448 * 2^e``).  ``enable_pdl`` is accepted and
ignored: there is no programmatic dependent launch on this hardware.  Nothing here keeps host state or synchronises,
so every call can be captured into a graph.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._mx import BLOCK, ceil_to, contiguous_aligned, linear_scales, sf_row_offset, sf_shape

def _check_input(input: torch.Tensor, alignment: int) -> None:
    _lib.require_gpu_tensor(input, "input")
    if input.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"input has dtype {input.dtype}, expected float16 or bfloat16")
    if input.dim() < 1:
        raise ValueError("input must have at least one dim")
    assert input.shape[-1] % BLOCK == 0
    if alignment <= 0 or alignment % BLOCK != 0:
        raise ValueError(f"alignment {alignment} must be a positive multiple of {BLOCK}")


def _quantize_into(x: torch.Tensor, q: torch.Tensor, sf: torch.Tensor, swizzled: bool, alignment: int,
                   m_indptr: Optional[torch.Tensor] = None) -> None:
    """fi_mxfp8_quantize on a 2-D ``x``; ``q`` and ``sf`` are the pre-allocated outputs (every byte of both is written)."""
    if x.shape[1] > 1 and x.stride(1) != 1 or x.stride(0) % 8 != 0 or x.data_ptr() % 16 != 0:
        x = x.contiguous()
    p = _lib.fi_mxfp8_quantize_params_t(
        input=x.data_ptr(), q=q.data_ptr(), sf=sf.data_ptr(), m_indptr=_lib.ptr(m_indptr),
        input_stride=x.stride(0) if x.shape[0] > 1 else x.shape[1], sf_bytes=sf.numel(), m=x.shape[0], k=x.shape[1],
        alignment=alignment, num_groups=0 if m_indptr is None else m_indptr.shape[0] - 1,
        sf_layout=_lib.FI_MX_SF_SWIZZLED_128X4 if swizzled else _lib.FI_MX_SF_LINEAR, dtype=_lib.fi_dtype(x.dtype))
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().fi_mxfp8_quantize(C.byref(p), _lib.current_stream(x.device)), "mxfp8_quantize")


def mxfp8_quantize(
    input: torch.Tensor,
    is_sf_swizzled_layout: bool = True,
    alignment: int = 32,
    enable_pdl: Optional[bool] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Quantise ``input`` (f16 / bf16 ``[..., k]``, ``k % 32 == 0``) to MXFP8 (ref: fp8_quantization.py:179-212).

    Returns ``(x_q, sf)``: ``x_q`` is float8_e4m3fn ``[..., k_pad]`` with ``k_pad`` = ``k`` rounded up to ``alignment``
    (a multiple of 32) and zeros in the padded columns; ``sf`` is a flat uint8 tensor, ``m * k_pad / 32`` bytes in the
    linear layout ``[m, k_pad / 32]`` or the swizzled "128x4" layout with rows padded to 128 and blocks to 4 (padding is
    0), where ``m`` is the product of the leading dims.
    """
    _check_input(input, alignment)
    k = input.shape[-1]
    m = input.numel() // k if k else 0
    k_pad = ceil_to(k, alignment)
    nkb = k_pad // BLOCK
    x_q = torch.empty((*input.shape[:-1], k_pad), dtype=torch.float8_e4m3fn, device=input.device)
    sf = torch.empty(sf_shape(m, nkb, bool(is_sf_swizzled_layout)), dtype=torch.uint8, device=input.device).view(-1)
    _quantize_into(input.reshape(m, k), x_q.view(m, k_pad), sf, bool(is_sf_swizzled_layout), alignment)
    return x_q, sf


def mxfp8_quantize_grouped(input: torch.Tensor, m_indptr: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Quantise the row operand of ``group_gemm_mxfp8_mxfp4_nt_groupwise``.  Not part of the reference: there the caller
    swizzles every group's scales and pads them to the grouped placement by hand.

    ``input`` is f16 / bf16 ``(cum_m, k)`` with ``k % 128 == 0``, ``m_indptr`` int32 ``(G + 1,)`` on the device (it is not
    read on the host).  Returns ``(x_q, a_scale)``: float8_e4m3fn ``(cum_m, k)`` and uint8
    ``((cum_m + 127 G) // 128 * 128, k // 32)`` in the grouped swizzled layout, padding as 0.
    Rows of no group (below ``m_indptr[0]``, at or past ``m_indptr[-1]``) are quantised too; they have no scale row.
    """
    _check_input(input, BLOCK)
    _lib.require_gpu_tensor(m_indptr, "m_indptr")
    if input.dim() != 2:
        raise ValueError(f"input must be 2D (cum_m, k), got shape {tuple(input.shape)}")
    if input.shape[1] % 128 != 0:
        raise ValueError(f"k = {input.shape[1]} must be a multiple of 128 for the grouped layout")
    if m_indptr.dtype != torch.int32 or m_indptr.dim() != 1 or m_indptr.shape[0] < 2:
        raise ValueError("m_indptr must be a 1D int32 tensor of G + 1 >= 2 entries")
    cum_m, k = input.shape
    x_q = torch.empty((cum_m, k), dtype=torch.float8_e4m3fn, device=input.device)
    a_scale = torch.empty(sf_shape(cum_m, k // BLOCK, groups=m_indptr.shape[0] - 1), dtype=torch.uint8, device=input.device)
    _quantize_into(input, x_q, a_scale, True, BLOCK, m_indptr.contiguous())
    return x_q, a_scale


def fp8_quantize_1x128(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Quantise activations to DeepSeek's fp8 block-scale format, the ``hidden_states`` / ``hidden_states_scale`` of
    ``trtllm_fp8_block_scale_moe``.  Not part of the reference, whose callers quantise in their own code.

    ``x`` is f16 / bf16 ``(T, H)`` with ``H % 128 == 0``.  Returns ``(q, scale)``: float8_e4m3fn ``(T, H)`` and float32
    ``(H // 128, T)`` contiguous.  Per row and block of 128 columns, in f32: ``s = max(amax / 448, 2^-126)`` and
    ``q = e4m3(clamp(x / s, -448, 448))`` rounded to nearest even; ``scale[kb, t] = s``.  ``amax / 448`` is the rule of the
    reference's kernel (csrc/trtllm_fused_moe_dev_kernel.cu:141-152); an all-zero block gets ``s = 2^-126`` and ``q = 0``.
    The gated activation of the layer quantises with the same device function (csrc/fp8_block_quant.h).
    """
    _lib.require_gpu_tensor(x, "x")
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"x has dtype {x.dtype}, expected float16 or bfloat16")
    if x.dim() != 2:
        raise ValueError(f"x must be 2D (T, H), got shape {tuple(x.shape)}")
    T, H = x.shape
    if H % 128 != 0:
        raise ValueError(f"H = {H} must be a multiple of 128")
    q = torch.empty((T, H), dtype=torch.float8_e4m3fn, device=x.device)
    scale = torch.empty((H // 128, T), dtype=torch.float32, device=x.device)
    if T == 0 or H == 0:
        return q, scale
    if x.stride(1) != 1 or x.stride(0) % 8 != 0 or x.data_ptr() % 16 != 0:
        x = contiguous_aligned(x, 16)
    p = _lib.fi_fp8_quantize_1x128_params_t(
        input=x.data_ptr(), q=q.data_ptr(), scale=scale.data_ptr(), input_stride=x.stride(0) if T > 1 else H, m=T, k=H,
        dtype=_lib.fi_dtype(x.dtype))
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().fi_fp8_quantize_1x128(C.byref(p), _lib.current_stream(x.device)), "fp8_quantize_1x128")
    return q, scale


def mxfp8_dequantize_host(
    input: torch.Tensor,
    scale_tensor: torch.Tensor,
    is_sf_swizzled_layout: bool = True,
) -> torch.Tensor:
    """``input`` (float8_e4m3fn, or its bytes as uint8, ``[m, k]``) times its block scales, as float32; pure torch on
    CPU tensors (ref: fp8_quantization.py:215-239)."""
    if input.is_cuda or scale_tensor.is_cuda:
        raise RuntimeError("mxfp8_dequantize_host works on CPU tensors (move them with .cpu())")
    if input.dim() != 2 or input.shape[1] % BLOCK != 0:
        raise ValueError(f"input must be 2D (m, k) with k a multiple of {BLOCK}, got shape {tuple(input.shape)}")
    if scale_tensor.dtype != torch.uint8:
        raise ValueError(f"scale_tensor has dtype {scale_tensor.dtype}, expected uint8")
    if input.dtype == torch.uint8:
        input = input.view(torch.float8_e4m3fn)
    m, k = input.shape
    nkb = k // BLOCK
    sf = linear_scales(scale_tensor, m, nkb, is_sf_swizzled_layout)
    scale = torch.exp2(sf.double() - 127.0).unsqueeze(-1)
    return (input.to(torch.float32).double().view(m, nkb, BLOCK) * scale).view(m, k).to(torch.float32)
