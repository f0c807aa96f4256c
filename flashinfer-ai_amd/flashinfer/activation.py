"""Gated activations of the MLP: ``act(input[..., :d]) * input[..., d:]`` for silu, gelu (erf) and gelu_tanh.
Mirrors flashinfer/activation.py (v0.3.1); the kernel is csrc/activation.hip behind fi_act_and_mul
(include/fi_mi355.h).  ``silu_and_mul_nvfp4_batched_quantize`` is not provided (fp4 is out of scope).

``input`` is f16 or bf16 of shape ``(..., 2 * d)``; an input that is not contiguous is made contiguous first.
``enable_pdl`` is accepted and ignored.  Nothing here keeps host state, so every call can be captured into a graph.
"""
from __future__ import annotations

import ctypes as C
import functools
from types import SimpleNamespace
from typing import Optional

import torch

from . import _lib

_ACT_CODES = {"silu": _lib.FI_ACT_SILU, "gelu": _lib.FI_ACT_GELU, "gelu_tanh": _lib.FI_ACT_GELU_TANH}


@functools.cache
def get_act_and_mul_module(act_func_name: str):
    """The reference's module getter (activation.py:65-88): a namespace whose ``<name>_and_mul(out, input,
    enable_pdl)`` writes ``out``."""
    try:
        code = _ACT_CODES[act_func_name]
    except KeyError:
        raise ValueError(f"unknown activation {act_func_name!r}; expected one of {sorted(_ACT_CODES)}") from None
    fname = f"{act_func_name}_and_mul"

    def _act_and_mul(out: torch.Tensor, input: torch.Tensor, enable_pdl: Optional[bool] = None) -> None:
        _lib.require_gpu_tensor(input, "input")
        _lib.require_gpu_tensor(out, "out")
        if out.dtype != input.dtype:
            raise ValueError(f"out has dtype {out.dtype}, expected {input.dtype}")
        if out.device != input.device:
            raise ValueError(f"out is on {out.device}, expected {input.device}")
        if input.dim() < 1 or input.shape[-1] % 2 != 0:
            raise ValueError(f"the last dim of input must be even (2 * hidden_size), got shape {tuple(input.shape)}")
        d = input.shape[-1] // 2
        if tuple(out.shape) != tuple(input.shape[:-1]) + (d,):
            raise ValueError(f"out has shape {tuple(out.shape)}, expected {tuple(input.shape[:-1]) + (d,)}")
        x = input.contiguous()
        o = out if out.is_contiguous() else torch.empty_like(out, memory_format=torch.contiguous_format)
        p = _lib.fi_act_and_mul_params_t(in_=x.data_ptr(), out=o.data_ptr(), tokens=o.numel() // d if d else 0, d=d, act=code,
                                 dtype=_lib.fi_dtype(input.dtype))
        with torch.cuda.device(input.device):
            _lib.check(_lib.lib().fi_act_and_mul(C.byref(p), _lib.current_stream(input.device)), fname)
        if o is not out:
            out.copy_(o)

    _act_and_mul.__name__ = fname
    return SimpleNamespace(**{fname: _act_and_mul})


def _check_shape(input: torch.Tensor, output: torch.Tensor) -> None:
    assert input.ndim == output.ndim, f"{input.ndim} != {output.ndim}"
    assert input.shape[:-1] == output.shape[:-1], f"{input.shape[:-1]} != {output.shape[:-1]}"
    assert input.shape[-1] == 2 * output.shape[-1], f"{input.shape[-1]} != {2 * output.shape[-1]}"


def _act_and_mul(name: str, input: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
    _lib.require_gpu_tensor(input, "input")
    if input.shape[-1] * input.dtype.itemsize % 16 != 0:
        raise ValueError("The pointers must be multiple of 16 bytes.")
    if out is not None:
        _check_shape(input, out)
    else:
        out = torch.empty(input.shape[:-1] + (input.shape[-1] // 2,), device=input.device, dtype=input.dtype)
    getattr(get_act_and_mul_module(name), f"{name}_and_mul")(out, input, None)
    return out


def silu_and_mul(input: torch.Tensor, out: torch.Tensor = None, enable_pdl: Optional[bool] = None) -> torch.Tensor:
    """``silu(input[..., :d]) * input[..., d:]`` (ref: activation.py:101-142)."""
    return _act_and_mul("silu", input, out)


def gelu_tanh_and_mul(input: torch.Tensor, out: torch.Tensor = None, enable_pdl: Optional[bool] = None) -> torch.Tensor:
    """``gelu_tanh(input[..., :d]) * input[..., d:]``, the tanh approximation (ref: activation.py:178-215)."""
    return _act_and_mul("gelu_tanh", input, out)


def gelu_and_mul(input: torch.Tensor, out: torch.Tensor = None, enable_pdl: Optional[bool] = None) -> torch.Tensor:
    """``gelu(input[..., :d]) * input[..., d:]`` with the erf form (ref: activation.py:218-255)."""
    return _act_and_mul("gelu", input, out)
