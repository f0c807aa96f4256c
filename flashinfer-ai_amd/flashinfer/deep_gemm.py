"""The reference's other spellings of the grouped fp8 GEMMs of expert-parallel MoE (ref: flashinfer/deep_gemm.py): the
names integrations call.  ``m_grouped_fp8_gemm_nt_masked`` forwards to
``flashinfer.gemm.batch_deepgemm_fp8_nt_groupwise`` (the masked layout of decode; kernel csrc/gemm_masked.hip) and
``m_grouped_fp8_gemm_nt_contiguous`` to ``flashinfer.gemm.group_deepgemm_fp8_nt_groupwise`` (the contiguous layout of
prefill; kernel csrc/gemm_contig.hip)."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .gemm import batch_deepgemm_fp8_nt_groupwise, group_deepgemm_fp8_nt_groupwise


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


def m_grouped_fp8_gemm_nt_contiguous(
    a_fp8: Tuple[torch.Tensor, torch.Tensor],  # (a (m, k), a_scale (m, k // 128))
    b_fp8: Tuple[torch.Tensor, torch.Tensor],  # (b (G, n, k), b_scale (G, n // 128, k // 128))
    d: torch.Tensor,  # (m, n) bf16 / fp16, written in place
    m_indices: torch.Tensor,  # (m,) int32 on the device
    recipe: Optional[Tuple[int, int, int]] = None,
    compiled_dims: str = "nk",
) -> None:
    """``d[r] = (a[r] * a_scale[r]) @ (b[g] * b_scale[g]).T`` with ``g = m_indices[128 (r // 128)]`` for every row of a
    live 128-row block whose own index is not negative, in place.  ``recipe`` is ``None`` or ``(1, 128, 128)``;
    ``compiled_dims`` is accepted and ignored."""
    a, a_scale = a_fp8
    b, b_scale = b_fp8
    group_deepgemm_fp8_nt_groupwise(a, b, a_scale, b_scale, m_indices,
                                    scale_granularity_mnk=(1, 128, 128) if recipe is None else recipe, out=d)
