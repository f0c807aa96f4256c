"""RMSNorm, Gemma RMSNorm and their fused residual-add forms.  Mirrors flashinfer/norm.py (v0.3.1) name by name and
argument by argument; the kernels are csrc/norm.hip behind fi_rmsnorm / fi_fused_add_rmsnorm (include/fi_mi355.h).

``input`` is f16 or bf16, 2-D ``(batch, hidden)`` or 3-D ``(batch, num_heads, head_dim)`` (the QK-norm of Qwen3 /
Gemma3) with a contiguous last dim and any row strides; ``weight`` is ``(hidden,)`` of the same dtype.  All arithmetic
is f32.  The Gemma forms are the same kernels with ``weight + 1``.  ``enable_pdl`` is accepted and ignored: there is
no programmatic dependent launch on this hardware.  Nothing here keeps host state, so every call can be captured
into a graph.
"""
from __future__ import annotations

import ctypes as C
import functools
from types import SimpleNamespace
from typing import Optional

import torch

from . import _lib


def _stride(t: torch.Tensor, dim: int, packed: int) -> int:
    """Element stride of ``dim``; a dim of size 1 is never stepped over, so it gets the packed stride."""
    return t.stride(dim) if t.shape[dim] > 1 else packed


def _check_rows(t: torch.Tensor, name: str, like: Optional[torch.Tensor] = None) -> None:
    _lib.require_gpu_tensor(t, name)
    if like is None:
        if t.dim() not in (2, 3):
            raise ValueError(f"{name} must be 2D (batch, hidden) or 3D (batch, num_heads, head_dim), got shape "
                             f"{tuple(t.shape)}")
    else:
        if t.shape != like.shape:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(like.shape)}")
        if t.dtype != like.dtype:
            raise ValueError(f"{name} has dtype {t.dtype}, expected {like.dtype}")
        if t.device != like.device:
            raise ValueError(f"{name} is on {t.device}, expected {like.device}")
    if t.shape[-1] > 1 and t.stride(-1) != 1:
        raise ValueError(f"the last dim of {name} must be contiguous (stride {t.stride(-1)})")


def _check_weight(weight: torch.Tensor, input: torch.Tensor) -> None:
    _lib.require_gpu_tensor(weight, "weight")
    if weight.dim() != 1 or weight.shape[0] != input.shape[-1]:
        raise ValueError(f"weight must be 1D of length {input.shape[-1]}, got shape {tuple(weight.shape)}")
    if weight.dtype != input.dtype:
        raise ValueError(f"weight has dtype {weight.dtype}, expected {input.dtype}")
    if weight.device != input.device:
        raise ValueError(f"weight is on {weight.device}, expected {input.device}")


def _rmsnorm_into(out: torch.Tensor, input: torch.Tensor, weight: torch.Tensor, eps: float, weight_bias: float,
                  what: str) -> None:
    _check_rows(input, "input")
    _check_rows(out, "out", input)
    _check_weight(weight, input)
    weight = weight.contiguous()
    hidden = input.shape[-1]
    if input.dim() == 2:
        heads, packed_n = 1, hidden
        strides = (_stride(input, 0, hidden), 0, _stride(out, 0, hidden), 0)
    else:
        heads, packed_n = input.shape[1], input.shape[1] * hidden
        strides = (_stride(input, 0, packed_n), _stride(input, 1, hidden), _stride(out, 0, packed_n),
                   _stride(out, 1, hidden))
    p = _lib.fi_rmsnorm_params_t(
        in_=input.data_ptr(), weight=weight.data_ptr(), out=out.data_ptr(), batch=input.shape[0], num_heads=heads,
        hidden=hidden, in_stride_n=strides[0], in_stride_h=strides[1], out_stride_n=strides[2],
        out_stride_h=strides[3], eps=float(eps), weight_bias=weight_bias, dtype=_lib.fi_dtype(input.dtype))
    with torch.cuda.device(input.device):
        _lib.check(_lib.lib().fi_rmsnorm(C.byref(p), _lib.current_stream(input.device)), what)


def _fused_add_rmsnorm(input: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float,
                       weight_bias: float, what: str) -> None:
    _lib.require_gpu_tensor(input, "input")
    if input.dim() != 2:
        raise ValueError(f"input must be 2D (batch, hidden), got shape {tuple(input.shape)}")
    _check_rows(input, "input")
    _check_rows(residual, "residual", input)
    _check_weight(weight, input)
    weight = weight.contiguous()
    hidden = input.shape[1]
    p = _lib.fi_fused_add_rmsnorm_params_t(
        input=input.data_ptr(), residual=residual.data_ptr(), weight=weight.data_ptr(), batch=input.shape[0],
        hidden=hidden, input_stride=_stride(input, 0, hidden), residual_stride=_stride(residual, 0, hidden),
        eps=float(eps), weight_bias=weight_bias, dtype=_lib.fi_dtype(input.dtype))
    with torch.cuda.device(input.device):
        _lib.check(_lib.lib().fi_fused_add_rmsnorm(C.byref(p), _lib.current_stream(input.device)), what)


@functools.cache
def get_norm_module():
    """The reference's module getter (norm.py:38-40): functions with the positional signatures of its exports
    (csrc/norm.cu:24-162), forwarding to the C ABI."""

    def rmsnorm(out, input, weight, eps, enable_pdl) -> None:
        """ref: csrc/norm.cu:24-79 (2-D: one workgroup per row; 3-D: one wave per (token, head) row)."""
        _rmsnorm_into(out, input, weight, eps, 0.0, "rmsnorm")

    def fused_add_rmsnorm(input, residual, weight, eps, enable_pdl) -> None:
        """ref: csrc/norm.cu:81-108."""
        _fused_add_rmsnorm(input, residual, weight, eps, 0.0, "fused_add_rmsnorm")

    def gemma_rmsnorm(out, input, weight, eps, enable_pdl) -> None:
        """ref: csrc/norm.cu:110-133."""
        _rmsnorm_into(out, input, weight, eps, 1.0, "gemma_rmsnorm")

    def gemma_fused_add_rmsnorm(input, residual, weight, eps, enable_pdl) -> None:
        """ref: csrc/norm.cu:135-162."""
        _fused_add_rmsnorm(input, residual, weight, eps, 1.0, "gemma_fused_add_rmsnorm")

    return SimpleNamespace(rmsnorm=rmsnorm, fused_add_rmsnorm=fused_add_rmsnorm, gemma_rmsnorm=gemma_rmsnorm,
                           gemma_fused_add_rmsnorm=gemma_fused_add_rmsnorm)


def rmsnorm(
    input: torch.Tensor,
    weight: torch.Tensor,
    eps: float = 1e-6,
    out: Optional[torch.Tensor] = None,
    enable_pdl: Optional[bool] = None,
) -> torch.Tensor:
    """``out[i] = input[i] / RMS(input) * weight[i]`` per row (ref: norm.py:43-78).  ``out`` may be ``input``."""
    if out is None:
        _lib.require_gpu_tensor(input, "input")
        out = torch.empty_like(input)
    get_norm_module().rmsnorm(out, input, weight, eps, enable_pdl)
    return out


def fused_add_rmsnorm(
    input: torch.Tensor,
    residual: torch.Tensor,
    weight: torch.Tensor,
    eps: float = 1e-6,
    enable_pdl: Optional[bool] = None,
) -> None:
    """``residual += input``, then ``input = residual / RMS(residual) * weight``, both in place (ref: norm.py:106-137).
    The norm is taken from the f32 sum before it is rounded into ``residual``."""
    get_norm_module().fused_add_rmsnorm(input, residual, weight, eps, enable_pdl)


def gemma_rmsnorm(
    input: torch.Tensor,
    weight: torch.Tensor,
    eps: float = 1e-6,
    out: Optional[torch.Tensor] = None,
    enable_pdl: Optional[bool] = None,
) -> torch.Tensor:
    """``out[i] = input[i] / RMS(input) * (weight[i] + 1)`` per row (ref: norm.py:151-186)."""
    if out is None:
        _lib.require_gpu_tensor(input, "input")
        out = torch.empty_like(input)
    get_norm_module().gemma_rmsnorm(out, input, weight, eps, enable_pdl)
    return out


def gemma_fused_add_rmsnorm(
    input: torch.Tensor,
    residual: torch.Tensor,
    weight: torch.Tensor,
    eps: float = 1e-6,
    enable_pdl: Optional[bool] = None,
) -> None:
    """``residual += input``, then ``input = residual / RMS(residual) * (weight + 1)`` (ref: norm.py:216-247)."""
    get_norm_module().gemma_fused_add_rmsnorm(input, residual, weight, eps, enable_pdl)
