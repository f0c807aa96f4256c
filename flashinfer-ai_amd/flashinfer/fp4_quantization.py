"""MXFP4 quantisation: the MX half of the reference's flashinfer/fp4_quantization.py (:525-830) -- ``fp4_quantize`` with
32-element blocks and UE8M0 scales, ``mxfp4_quantize``, ``block_scale_interleave``, the host dequantisers -- and
``mxfp4_quantize_grouped``, this project's own extension that returns the ``b`` / ``b_scale`` of
``group_gemm_mxfp8_mxfp4_nt_groupwise``.  The kernels are csrc/mxfp4_quantize.hip behind fi_mxfp4_quantize and
fi_mx_sf_interleave (include/fi_mi355.h).

An MXFP4 tensor is e2m1 codes, two per byte with element ``2i`` in the low nibble of byte ``i``, plus one E8M0 byte
(value ``2^(byte - 127)``) per 32 consecutive elements of a row.  The scale of a block is the smallest power of two
``2^e`` with ``6 * 2^e >= amax``; the compare is exact (the reference's approximate reciprocal may give ``e + 1`` at
``amax == 6 * 2^e``), and the codes are ``x * 2^-e`` rounded to nearest, ties to even.  The sign nibble of a value that
rounds to zero is unspecified; NaN / Inf inputs and magnitudes below ``2^-126`` are outside the contract.

nvfp4 (16-element blocks, e4m3 scales, a global scale) and the 8x4 scale layout are not provided:
every call that selects them raises NotImplementedError.  ``global_scale`` and ``enable_pdl`` are accepted and ignored:
the reference does not use the former with UE8M0 scales, and there is no programmatic dependent launch on this
hardware.  Nothing here keeps host state or synchronises, so every device call can be captured into a graph.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._mx import BLOCK, linear_scales, sf_shape

_E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _quantize_into(x: torch.Tensor, q: torch.Tensor, sf: torch.Tensor, num_groups: int, swizzled: bool) -> None:
    """fi_mxfp4_quantize on a 2-D ``x`` of ``num_groups`` equal row groups; every byte of ``q`` and ``sf`` is written."""
    if x.shape[1] > 1 and x.stride(1) != 1 or x.stride(0) % 8 != 0 or x.stride(0) < x.shape[1] or x.data_ptr() % 16 != 0:
        x = x.contiguous()
    p = _lib.fi_mxfp4_quantize_params_t(
        input=x.data_ptr(), q=q.data_ptr(), sf=sf.data_ptr(),
        input_stride=x.stride(0) if x.shape[0] > 1 else x.shape[1], sf_bytes=sf.numel(), num_groups=num_groups,
        rows=x.shape[0] // max(num_groups, 1), k=x.shape[1],
        sf_layout=_lib.FI_MX_SF_SWIZZLED_128X4 if swizzled else _lib.FI_MX_SF_LINEAR, dtype=_lib.fi_dtype(x.dtype))
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().fi_mxfp4_quantize(C.byref(p), _lib.current_stream(x.device)), "mxfp4_quantize")


def _check_input(input: torch.Tensor) -> None:
    _lib.require_gpu_tensor(input, "input")
    if input.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"input has dtype {input.dtype}, expected float16 or bfloat16")


def fp4_quantize(
    input: torch.Tensor,
    global_scale: Optional[torch.Tensor] = None,
    sf_vec_size: int = 16,
    sf_use_ue8m0: bool = False,
    is_sf_swizzled_layout: bool = True,
    is_sf_8x4_layout: bool = False,
    enable_pdl: Optional[bool] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Quantise ``input`` (f16 / bf16 ``[..., k]``, ``k % 32 == 0``) to MXFP4 (ref: fp4_quantization.py:525-587).

    Only ``sf_vec_size == 32 and sf_use_ue8m0 and not is_sf_8x4_layout`` runs; the defaults select nvfp4, which is not
    provided, so a bare call raises NotImplementedError.  Returns ``(x_q, sf)``: ``x_q`` uint8 ``[..., k / 2]`` and ``sf``
    uint8 reshaped to ``(-1, k / 32)`` -- ``[m, k / 32]`` in the linear layout, and the swizzled "128x4" bytes (rows padded
    to 128, blocks to 4, padding 0) in the swizzled one, which therefore needs ``ceil(m / 128) * 128 * ceil(k / 128) * 4``
    to be a multiple of ``k / 32``.  ``m`` is the product of the leading dims.  A column-major ``input``
    (``input.stride(-2) == 1``) is quantised along its contiguous dim and both results are returned transposed.
    """
    if sf_vec_size != 16 and sf_vec_size != 32:
        raise NotImplementedError("sf_vec_size can only be 16 or 32")
    if sf_vec_size != 32 or not sf_use_ue8m0:
        raise NotImplementedError(
            "nvfp4 (sf_vec_size 16, e4m3 scales, global scale) is not provided: only MXFP4, sf_vec_size=32 with "
            "sf_use_ue8m0=True, runs on this hardware")
    if is_sf_8x4_layout:
        raise NotImplementedError("the 8x4 layout of the scales is not provided: only linear and 128x4")
    _check_input(input)
    if input.dim() < 1:
        raise ValueError("input must have at least one dim")

    is_column_major = input.dim() >= 2 and input.stride(-2) == 1
    if is_column_major:
        input = input.transpose(-2, -1)
    k = input.shape[-1]
    assert k % sf_vec_size == 0
    m = input.numel() // k if k else 0
    nkb = k // BLOCK
    sf_rows, sf_blocks = sf_shape(m, nkb, bool(is_sf_swizzled_layout))
    sf_size = sf_rows * sf_blocks
    if nkb and sf_size % nkb != 0:
        raise ValueError(f"{sf_size} swizzled scale bytes do not reshape to (-1, {nkb}): use k % 128 == 0 or the linear layout")
    x_q = torch.empty((*input.shape[:-1], k // 2), dtype=torch.uint8, device=input.device)
    sf = torch.empty((sf_size,), dtype=torch.uint8, device=input.device)
    _quantize_into(input.reshape(m, k), x_q.view(m, k // 2), sf, 1, bool(is_sf_swizzled_layout))
    sf = sf.reshape((sf_size // nkb if nkb else 0, nkb))  # the reference's reshape((-1, k / 32)), also when empty
    if is_column_major:
        x_q = x_q.transpose(-2, -1)
        sf = sf.transpose(-2, -1)
    return x_q, sf


def mxfp4_quantize(a: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``fp4_quantize(a, None, 32, True, True)`` (ref: fp4_quantization.py:767-781).  The reference first derives a global
    scale from ``a.max()`` that its MX kernel then ignores; there is no such reduction and no host sync here."""
    return fp4_quantize(a, None, 32, True, True)


def mxfp4_quantize_grouped(input: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Quantise the weight operand of ``group_gemm_mxfp8_mxfp4_nt_groupwise``.  Not part of the reference: there the
    caller quantises and swizzles every group by hand.

    ``input`` is f16 / bf16 ``(G, n, k)`` with ``k % 128 == 0``.  Returns ``(b, b_scale)``: uint8 ``(G, n, k / 2)`` and uint8
    ``(G, ceil(n / 128) * 128, k / 32)`` with every group swizzled on its own, padding as 0.
    """
    _check_input(input)
    if input.dim() != 3:
        raise ValueError(f"input must be 3D (G, n, k), got shape {tuple(input.shape)}")
    G, n, k = input.shape
    if k % 128 != 0:
        raise ValueError(f"k = {k} must be a multiple of 128 for the grouped layout")
    b = torch.empty((G, n, k // 2), dtype=torch.uint8, device=input.device)
    b_scale = torch.empty((G, *sf_shape(n, k // BLOCK)), dtype=torch.uint8, device=input.device)
    _quantize_into(input.reshape(G * n, k), b.view(G * n, k // 2), b_scale, G, True)
    return b, b_scale


def block_scale_interleave(unswizzled_sf: torch.Tensor) -> torch.Tensor:
    """Linear scale bytes ``[rows, cols]`` or ``[groups, rows, cols]`` (uint8) -> the flat swizzled "128x4" tensor of
    ``groups * ceil(rows / 128) * 128 * ceil(cols / 4) * 4`` bytes, every group on its own, padding as 0
    (ref: fp4_quantization.py:590-615)."""
    assert unswizzled_sf.dtype == torch.uint8, f"Input dtype must be uint8, got {unswizzled_sf.dtype}"
    _lib.require_gpu_tensor(unswizzled_sf, "unswizzled_sf")
    if unswizzled_sf.dim() not in (2, 3):
        raise ValueError(f"unswizzled_sf must be 2D or 3D, got shape {tuple(unswizzled_sf.shape)}")
    x = unswizzled_sf.contiguous()
    rows, cols = x.shape[-2:]
    groups = x.shape[0] if x.dim() == 3 else 1
    out = torch.empty((groups, *sf_shape(rows, cols)), dtype=torch.uint8, device=x.device).view(-1)
    p = _lib.fi_mx_sf_interleave_params_t(input=x.data_ptr(), output=out.data_ptr(), output_bytes=out.numel(),
                                          num_groups=groups, rows=rows, cols=cols)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().fi_mx_sf_interleave(C.byref(p), _lib.current_stream(x.device)), "block_scale_interleave")
    return out


# the reference keeps the old name
nvfp4_block_scale_interleave = block_scale_interleave


def _e2m1_to_float(packed: torch.Tensor) -> torch.Tensor:
    """uint8 ``[m, k / 2]`` -> float64 ``[m, k]``."""
    codes = torch.stack([packed & 15, packed >> 4], dim=-1).flatten(-2).long()
    mag = torch.tensor(_E2M1_VALUES, dtype=torch.float64)[codes & 7]
    return torch.where((codes & 8) != 0, -mag, mag)


def _dequantize(packed: torch.Tensor, sf: torch.Tensor) -> torch.Tensor:
    """codes ``[m, k / 2]`` times the scale bytes ``[m, k / 32]``, as float32 (every product is exact in float64)."""
    m, k = packed.shape[0], packed.shape[1] * 2
    scale = torch.exp2(sf.double() - 127.0).unsqueeze(-1)
    return (_e2m1_to_float(packed).view(m, k // BLOCK, BLOCK) * scale).view(m, k).to(torch.float32)


def e2m1_and_ufp8sf_scale_to_float(
    e2m1_tensor: torch.Tensor,
    ufp8_scale_tensor: torch.Tensor,
    global_scale_tensor: Optional[torch.Tensor] = None,
    sf_vec_size: int = 16,
    ufp8_type: int = 1,
    is_sf_swizzled_layout: bool = True,
) -> torch.Tensor:
    """Packed e2m1 ``[m, k / 2]`` (uint8) times its UE8M0 block scales, as float32; pure torch on CPU tensors
    (ref: fp4_quantization.py:622-661).  Only ``sf_vec_size == 32, ufp8_type == 0`` runs: e4m3 scales over 16 elements
    are nvfp4, which is not provided.  ``global_scale_tensor`` is accepted and ignored, as MX has none."""
    if sf_vec_size != 32 or ufp8_type != 0:
        raise NotImplementedError(
            "nvfp4 (sf_vec_size 16, e4m3 scales: ufp8_type 1) is not provided: only sf_vec_size=32 with ufp8_type=0")
    if e2m1_tensor.is_cuda or ufp8_scale_tensor.is_cuda:
        raise RuntimeError("e2m1_and_ufp8sf_scale_to_float works on CPU tensors (move them with .cpu())")
    if e2m1_tensor.dtype != torch.uint8 or ufp8_scale_tensor.dtype != torch.uint8:
        raise ValueError("e2m1_tensor and ufp8_scale_tensor must be uint8")
    if e2m1_tensor.dim() != 2 or e2m1_tensor.shape[1] % (BLOCK // 2) != 0:
        raise ValueError(f"e2m1_tensor must be 2D (m, k / 2) with k a multiple of {BLOCK}, got shape {tuple(e2m1_tensor.shape)}")
    m, nkb = e2m1_tensor.shape[0], e2m1_tensor.shape[1] * 2 // BLOCK
    return _dequantize(e2m1_tensor, linear_scales(ufp8_scale_tensor, m, nkb, is_sf_swizzled_layout))


def mxfp4_dequantize(a_fp4: torch.Tensor, a_sf: torch.Tensor) -> torch.Tensor:
    """The float32 values of ``mxfp4_quantize``'s results (swizzled scales), computed on the CPU as in the reference
    (fp4_quantization.py:784-802)."""
    return e2m1_and_ufp8sf_scale_to_float(
        a_fp4.cpu().view(torch.uint8), a_sf.cpu().view(torch.uint8).reshape(-1), None, 32, 0, True)


def mxfp4_dequantize_host(
    weight: torch.Tensor,
    scale: torch.Tensor,
    group_size: int = 32,
) -> torch.Tensor:
    """``weight`` (uint8 ``[m, k / 2]``) times its linear scales (uint8 ``[m, k / 32]``), as float32; pure torch on CPU
    tensors (ref: fp4_quantization.py:805-830)."""
    if group_size != BLOCK:
        raise NotImplementedError(f"group_size {group_size}: MXFP4 has blocks of {BLOCK}")
    if weight.is_cuda or scale.is_cuda:
        raise RuntimeError("mxfp4_dequantize_host works on CPU tensors (move them with .cpu())")
    if weight.dtype != torch.uint8 or scale.dtype != torch.uint8:
        raise ValueError("weight and scale must be uint8")
    if weight.dim() != 2 or weight.shape[1] % (BLOCK // 2) != 0:
        raise ValueError(f"weight must be 2D (m, k / 2) with k a multiple of {BLOCK}, got shape {tuple(weight.shape)}")
    m, nkb = weight.shape[0], weight.shape[1] * 2 // BLOCK
    if scale.numel() != m * nkb:
        raise ValueError(f"scale holds {scale.numel()} bytes, {m * nkb} needed")
    return _dequantize(weight, scale.reshape(m, nkb))
