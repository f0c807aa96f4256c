"""Where the E8M0 scale bytes of an MX operand live and how many there are: the Python side of csrc/mx_layout.h, which
describes the layouts, shared by fp8_quantization.py, fp4_quantization.py and fused_moe.py (gemm.py passes the buffers on
and leaves the check of their sizes to the C entry).  One scale byte covers ``BLOCK`` consecutive k elements of a row."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

BLOCK = 32


def ceil_to(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def sf_offset(r: torch.Tensor, kb: torch.Tensor, nkb: int) -> torch.Tensor:
    """Byte of (row, k block) in the swizzled "128x4" layout (include/fi_mi355.h, csrc/mx_layout.h)."""
    return (r // 128) * ((nkb + 3) // 4) * 512 + (kb // 4) * 512 + (r % 32) * 16 + ((r % 128) // 32) * 4 + kb % 4


def sf_row_offset(m_begin: int, group: int) -> int:
    """First scale row of ``group`` whose rows start at ``m_begin`` in the grouped layout; ``sf_row_offset(cum_m, G)`` is
    the row count of the whole scale tensor."""
    return (m_begin + 127 * group) // 128 * 128


def sf_shape(m: int, nkb: int, swizzled: bool = True, groups: Optional[int] = None) -> Tuple[int, int]:
    """(rows, k blocks) of the scale tensor of ``m`` rows of ``nkb`` blocks, padding included: linear, swizzled, or with
    ``groups`` the grouped layout of ``m`` rows in that many groups."""
    if not swizzled:
        return m, nkb
    return ceil_to(m, 128) if groups is None else sf_row_offset(m, groups), ceil_to(nkb, 4)


def linear_scales(scale_tensor: torch.Tensor, m: int, nkb: int, swizzled: bool) -> torch.Tensor:
    """The ``[m, nkb]`` scale bytes of a CPU scale tensor in the linear or the swizzled layout (padding is not read)."""
    flat = scale_tensor.reshape(-1)
    rows, blocks = sf_shape(m, nkb, swizzled)
    need = rows * blocks
    if flat.numel() < need:
        raise ValueError(f"the scale tensor holds {flat.numel()} bytes, {need} needed")
    if not swizzled:
        return flat[: m * nkb].view(m, nkb)
    r = torch.arange(m).view(-1, 1).expand(m, nkb)
    kb = torch.arange(nkb).view(1, -1).expand(m, nkb)
    return flat[sf_offset(r, kb, nkb).reshape(-1)].view(m, nkb)


def scale_bytes(t: torch.Tensor) -> torch.Tensor:
    """E8M0 scale bytes given as uint8 or float8_e4m3fn: either is read as bytes."""
    return t if t.dtype == torch.uint8 else t.view(torch.uint8)


def contiguous_aligned(t: torch.Tensor, alignment: int) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % alignment == 0 else t.clone()
