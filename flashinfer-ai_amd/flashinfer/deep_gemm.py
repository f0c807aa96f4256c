"""The reference's other spelling of the masked batched fp8 GEMM (ref: flashinfer/deep_gemm.py,
``m_grouped_fp8_gemm_nt_masked``): the name integrations call.  It forwards to
``flashinfer.gemm.batch_deepgemm_fp8_nt_groupwise``; the kernel is csrc/gemm_masked.hip."""
from __future__ import annotations

from typing import Tuple

import torch

from .gemm import batch_deepgemm_fp8_nt_groupwise


def m_grouped_fp8_gemm_nt_masked(
    a_fp8: Tuple[torch.Tensor, torch.Tensor],  # (a (E, m, k), a_scale (E, m, k // 128))
    b_fp8: Tuple[torch.Tensor, torch.Tensor],  # (b (E, n, k), b_scale (E, n // 128, k // 128))
    d: torch.Tensor,  # (E, m, n) bf16 / fp16, written in place
    masked_m: torch.Tensor,  # (E,) int32 on the device
    expected_m: int,
    scale_granularity_mnk: Tuple[int, int, int] = (1, 128, 128),
) -> None:
    """``d[e, :masked_m[e]] = (a[e] * a_scale[e]) @ (b[e] * b_scale[e]).T`` for every expert, in place."""
    a, a_scale = a_fp8
    b, b_scale = b_fp8
    batch_deepgemm_fp8_nt_groupwise(a, b, a_scale, b_scale, masked_m, expected_m,
                                    scale_granularity_mnk=scale_granularity_mnk, out=d)
