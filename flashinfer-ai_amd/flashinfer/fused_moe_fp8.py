"""``trtllm_fp8_block_scale_moe`` of the reference's flashinfer/fused_moe/core.py (:1742-1816): the mixture-of-experts layer on
DeepSeek's fp8 block-scale format -- e4m3 weights with one f32 scale per 128 x 128 block, e4m3 activations with one per
token and 128 columns, as DeepSeek-V3 / R1 checkpoints ship.

The layer is the six steps of ``flashinfer.fused_moe`` on that format: ``moe_route``, ``moe_permute_fp8_block``, GEMM1,
``moe_gated_act_fp8_block`` (plain SwiGLU), GEMM2, ``moe_finalize`` -- the stage functions live in ``flashinfer.fused_moe``
(csrc/moe.hip), the GEMMs are ``group_gemm_fp8_nt_groupwise`` (csrc/gemm.hip, gemm_big.hip) in its ``"K"`` scale mode, and
``flashinfer.fp8_quantization.fp8_quantize_1x128`` makes the activations.  The call is a module of its own, reached as
``flashinfer.fused_moe_fp8.trtllm_fp8_block_scale_moe``: ``flashinfer.fused_moe`` and the package's top level hold the
MXFP4 layer's names only.  Shuffled weights and the BlockMajorK layout are NVIDIA kernel layouts and are
refused; ``trtllm_fp8_per_tensor_scale_moe`` is not provided.

Nothing here reads a device value on the host or synchronises, and every buffer's size depends on shapes alone, so a
call can be captured into a graph.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .fused_moe import (_check_fp8_block_activations, _check_routing, moe_finalize, moe_gated_act_fp8_block,
                        moe_permute_fp8_block, moe_route)
from .gemm import _group_gemm_fp8_into

_FP8_BLOCK = 128


def _check_fp8_block_weights(name: str, w: torch.Tensor, scale: torch.Tensor, G: int, n: int, k: int) -> None:
    if w.dtype != torch.float8_e4m3fn or tuple(w.shape) != (G, n, k):
        raise NotImplementedError(f"{name} must be float8_e4m3fn of shape ({G}, {n}, {k}) (MajorK, not shuffled), got "
                                  f"{w.dtype} {tuple(w.shape)}")
    want = (G, n // _FP8_BLOCK, k // _FP8_BLOCK)
    if scale.dtype != torch.float32 or tuple(scale.shape) != want:
        raise NotImplementedError(f"{name}_scale must be float32 of shape {want} (one scale per 128 x 128 block), got "
                                  f"{scale.dtype} {tuple(scale.shape)}")


def trtllm_fp8_block_scale_moe(
    routing_logits: torch.Tensor,
    routing_bias: Optional[torch.Tensor],
    hidden_states: torch.Tensor,
    hidden_states_scale: torch.Tensor,
    gemm1_weights: torch.Tensor,
    gemm1_weights_scale: torch.Tensor,
    gemm2_weights: torch.Tensor,
    gemm2_weights_scale: torch.Tensor,
    num_experts: int,
    top_k: int,
    n_group: Optional[int],
    topk_group: Optional[int],
    intermediate_size: int,
    local_expert_offset: int,
    local_num_experts: int,
    routed_scaling_factor: Optional[float],
    tile_tokens_dim: int = 8,
    routing_method_type: int = 0,
    use_shuffled_weight: bool = False,
    weight_layout: int = 0,
    enable_pdl: Optional[bool] = None,
) -> torch.Tensor:
    """MoE layer on DeepSeek's fp8 block-scale format (ref: flashinfer/fused_moe/core.py:1742-1816): e4m3 weights with one
    f32 scale per 128 x 128 block, e4m3 activations with one per token and 128 columns.

    routing_logits : ``[T, num_experts]`` f32 / bf16, ``num_experts <= 512``, ``1 <= top_k <= min(8, num_experts)``.
    hidden_states, hidden_states_scale : float8_e4m3fn ``[T, H]`` and float32 ``[H / 128, T]`` with any strides (the
        reference's test passes ``.t()`` of a ``[T, H / 128]`` tensor; nothing is copied) -- ``fp8_quantize_1x128(x)`` makes
        both.  ``H % 128 == 0``.
    gemm1_weights, gemm1_weights_scale : float8_e4m3fn ``[E_local, 2 I, H]`` and float32 ``[E_local, 2 I / 128, H / 128]``;
        rows ``[0, I)`` produce the linear half, ``[I, 2 I)`` the gate.  ``I % 128 == 0``.
    gemm2_weights, gemm2_weights_scale : float8_e4m3fn ``[E_local, H, I]`` and float32 ``[E_local, H / 128, I / 128]``.
    routing_method_type, routing_bias, n_group, topk_group, routed_scaling_factor : as ``trtllm_fp4_block_scale_moe``
        (``moe_route``): every method but Unspecified; the four DeepSeekV3 arguments only with that method.
    use_shuffled_weight, weight_layout : False and 0 (MajorK); the shuffle and BlockMajorK are NVIDIA kernel layouts.
    tile_tokens_dim, enable_pdl : validated, then ignored.

    Returns bf16 ``[T, H]``; a token without a local expert gets zeros.  The steps are ``moe_route``,
    ``moe_permute_fp8_block``, the grouped fp8 GEMM, ``moe_gated_act_fp8_block`` (plain SwiGLU), the GEMM again and
    ``moe_finalize``: the result is bit for bit what calling them by hand gives.  GEMM1's output is rounded to bf16 before the
    activation.  Nothing is read back to the host and nothing synchronises: the call can be captured into a graph.
    """
    # ---- what is not provided, before anything touches the device ----
    if use_shuffled_weight:
        raise NotImplementedError("use_shuffled_weight=True is not provided: the weight shuffle is an NVIDIA kernel layout, "
                                  "pass the weights as the checkpoint has them")
    if int(weight_layout) != 0:
        raise NotImplementedError(f"weight_layout {weight_layout} is not provided: only 0 (MajorK)")
    if isinstance(tile_tokens_dim, bool) or not isinstance(tile_tokens_dim, int) or tile_tokens_dim <= 0:
        raise ValueError(f"tile_tokens_dim must be a positive int, got {tile_tokens_dim!r}")
    if enable_pdl is not None and not isinstance(enable_pdl, bool):
        raise ValueError(f"enable_pdl must be None or a bool, got {enable_pdl!r}")
    _check_routing(routing_method_type, top_k, num_experts, routing_bias, n_group, topk_group, routed_scaling_factor)
    _check_fp8_block_activations(hidden_states, hidden_states_scale)
    T, H = hidden_states.shape
    I, G = intermediate_size, local_num_experts
    if I <= 0 or I % _FP8_BLOCK != 0:
        raise NotImplementedError(f"intermediate_size {I} must be a multiple of 128 (pad it)")
    if local_expert_offset < 0 or G < 1 or local_expert_offset + G > num_experts:
        raise ValueError(f"the local experts [{local_expert_offset}, {local_expert_offset + G}) are not within "
                         f"[0, num_experts = {num_experts})")
    _check_fp8_block_weights("gemm1_weights", gemm1_weights, gemm1_weights_scale, G, 2 * I, H)
    _check_fp8_block_weights("gemm2_weights", gemm2_weights, gemm2_weights_scale, G, H, I)
    if routing_logits.dim() != 2 or tuple(routing_logits.shape) != (T, num_experts):
        raise ValueError(f"routing_logits must have shape ({T}, {num_experts}), got {tuple(routing_logits.shape)}")
    if routing_logits.dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError(f"routing_logits has dtype {routing_logits.dtype}: only float32 and bfloat16")
    weights = [("gemm1_weights", gemm1_weights), ("gemm1_weights_scale", gemm1_weights_scale),
               ("gemm2_weights", gemm2_weights), ("gemm2_weights_scale", gemm2_weights_scale)]
    for name, t in weights:
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous: there is no silent copy of a weight tensor")
    for name, t in [("routing_logits", routing_logits), ("routing_bias", routing_bias), ("hidden_states", hidden_states),
                    ("hidden_states_scale", hidden_states_scale)] + weights:
        if t is not None:
            _lib.require_gpu_tensor(t, name)
    dev = hidden_states.device
    if T == 0:
        return torch.empty((0, H), dtype=torch.bfloat16, device=dev)

    # ---- the layer ----
    ids, expert_weights = moe_route(routing_logits, top_k, routing_method_type, routing_bias=routing_bias,
                                    n_group=n_group, topk_group=topk_group, routed_scaling_factor=routed_scaling_factor)
    m_indptr, emap, x_perm, scale_perm = moe_permute_fp8_block(ids, hidden_states, hidden_states_scale,
                                                               local_expert_offset, G)
    n = T * top_k
    gemm1_output = torch.empty((n, 2 * I), dtype=torch.bfloat16, device=dev)
    _group_gemm_fp8_into(x_perm, gemm1_weights, scale_perm, gemm1_weights_scale, gemm1_output, m_indptr)
    act, act_scale = moe_gated_act_fp8_block(gemm1_output, m_indptr)
    gemm2_output = torch.empty((n, H), dtype=torch.bfloat16, device=dev)
    _group_gemm_fp8_into(act, gemm2_weights, act_scale, gemm2_weights_scale, gemm2_output, m_indptr)
    return moe_finalize(gemm2_output, expert_weights, emap)
