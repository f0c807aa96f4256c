"""``cutlass_fused_moe`` of the reference's flashinfer/fused_moe/core.py (:758-786) in its unquantised mode: the mixture-of-experts
layer on f16 / bf16 activations and weights, the call vLLM and SGLang make for Mixtral, Qwen-MoE and any checkpoint served
in 16 bits.  The caller routes (``token_selected_experts``, ``token_final_scales``).

The layer is four stages of ``flashinfer.fused_moe``: ``moe_sort``, ``moe_group_gemm_16bit`` (csrc/gemm_16bit.hip; it gathers
its rows by the sorted list in its own loads and applies SwiGLU in its epilogue), the same GEMM again and
``moe_finalize_16bit``.  The call is a module of its own, reached as ``flashinfer.fused_moe_16bit.cutlass_fused_moe``:
``flashinfer.fused_moe`` and the package's top level hold the MXFP4 layer's names only.  The fp8, nvfp4 and
W4A8 modes of the call, expert biases and all-to-all are refused by name.

Nothing here reads a device value on the host or synchronises, and every buffer's size depends on shapes alone, so a
call can be captured into a graph.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from . import _lib
from .fused_moe import (_16BIT, _MAX_EXPERTS, _MAX_TOP_K, _check_output_16bit, moe_finalize_16bit, moe_group_gemm_16bit,
                        moe_sort)


def cutlass_fused_moe(
    input: torch.Tensor,
    token_selected_experts: torch.Tensor,
    token_final_scales: torch.Tensor,
    fc1_expert_weights: torch.Tensor,
    fc2_expert_weights: torch.Tensor,
    output_dtype: torch.dtype,
    quant_scales: Optional[List[torch.Tensor]],
    fc1_expert_biases: Optional[torch.Tensor] = None,
    fc2_expert_biases: Optional[torch.Tensor] = None,
    input_sf: Optional[torch.Tensor] = None,
    swiglu_alpha: Optional[torch.Tensor] = None,
    swiglu_beta: Optional[torch.Tensor] = None,
    swiglu_limit: Optional[torch.Tensor] = None,
    tp_size: int = 1,
    tp_rank: int = 0,
    ep_size: int = 1,
    ep_rank: int = 0,
    cluster_size: int = 1,
    cluster_rank: int = 0,
    output: Optional[torch.Tensor] = None,
    enable_alltoall: bool = False,
    use_deepseek_fp8_block_scale: bool = False,
    use_w4_group_scaling: bool = False,
    use_mxfp8_act_scaling: bool = False,
    min_latency_mode: bool = False,
    tune_max_num_tokens: int = 8192,
    enable_pdl: Optional[bool] = None,
) -> List[torch.Tensor]:
    """MoE layer on unquantised f16 / bf16 weights (ref: flashinfer/fused_moe/core.py:758-786), the call vLLM and SGLang make
    for Mixtral, Qwen-MoE and any checkpoint served in 16 bits.

    input : f16 / bf16 ``[T, H]``, ``H % 64 == 0``.
    token_selected_experts, token_final_scales : int32 ``[T, top_k]`` of global expert ids and float32 ``[T, top_k]``; the
        caller routes.  ``top_k <= 8``.
    fc1_expert_weights : ``[E_local, 2 I, H]`` of the input's dtype, rows ``[0, I)`` the linear half (w3) and ``[I, 2 I)`` the
        gate (w1), the reference's layout; ``I % 64 == 0``.  fc2_expert_weights : ``[E_local, H, I]``.
    output_dtype : the input's dtype.  quant_scales : None or empty.
    swiglu_alpha, swiglu_beta, swiglu_limit : f32 ``[E_local]``, all three or none (``moe_group_gemm_16bit``).
    ep_size, ep_rank : the local experts are the global ids ``[ep_rank * E_local, (ep_rank + 1) * E_local)``; a slot on
        another expert contributes nothing, a token without a local slot gets zeros.
    tp_size, tp_rank : accepted; the weights arrive sliced.  cluster_size, cluster_rank, tune_max_num_tokens, enable_pdl :
        accepted and ignored.
    output : optional contiguous ``[T, H]`` tensor of the input's dtype.

    Biases, ``input_sf``, quantised inputs or weights, ``enable_alltoall``, ``use_deepseek_fp8_block_scale``,
    ``use_w4_group_scaling``, ``use_mxfp8_act_scaling`` and ``min_latency_mode`` raise NotImplementedError.

    Returns ``[out]``, as the reference's module does.  Four stages without a synchronisation between them --
    ``moe_sort``, ``moe_group_gemm_16bit`` gathering ``input`` by the sorted rows with SwiGLU in its epilogue, the GEMM
    again, ``moe_finalize_16bit`` -- and the result is bit for bit what calling them by hand gives.
    """
    # ---- what is not provided, before anything touches the device ----
    for name, t in (("fc1_expert_biases", fc1_expert_biases), ("fc2_expert_biases", fc2_expert_biases),
                    ("input_sf", input_sf)):
        if t is not None:
            raise NotImplementedError(f"{name} is not provided: pass None")
    for name, flag in (("enable_alltoall", enable_alltoall), ("use_deepseek_fp8_block_scale", use_deepseek_fp8_block_scale),
                       ("use_w4_group_scaling", use_w4_group_scaling), ("use_mxfp8_act_scaling", use_mxfp8_act_scaling),
                       ("min_latency_mode", min_latency_mode)):
        if flag:
            raise NotImplementedError(f"{name}=True is not provided")
    if quant_scales is not None and len(quant_scales) != 0:
        raise NotImplementedError("quant_scales is not provided: the fp8 / nvfp4 / W4A8 modes of this call are not, pass None")
    for name, t in (("input", input), ("fc1_expert_weights", fc1_expert_weights), ("fc2_expert_weights", fc2_expert_weights)):
        if t.dtype not in _16BIT:
            raise NotImplementedError(f"{name} has dtype {t.dtype}: only float16 and bfloat16 (unquantised) are provided")
    dtype = input.dtype
    if fc1_expert_weights.dtype != dtype or fc2_expert_weights.dtype != dtype or output_dtype != dtype:
        raise ValueError(f"input is {dtype}: the weights ({fc1_expert_weights.dtype}, {fc2_expert_weights.dtype}) and "
                         f"output_dtype ({output_dtype}) must be the same")
    if input.dim() != 2 or fc1_expert_weights.dim() != 3 or fc2_expert_weights.dim() != 3:
        raise ValueError("input must be 2D (T, H), fc1_expert_weights (E_local, 2 I, H) and fc2_expert_weights (E_local, H, I)")
    T, H = input.shape
    G, two_i, _ = fc1_expert_weights.shape
    I = two_i // 2
    if tuple(fc1_expert_weights.shape) != (G, 2 * I, H) or tuple(fc2_expert_weights.shape) != (G, H, I):
        raise ValueError(f"fc1_expert_weights {tuple(fc1_expert_weights.shape)} and fc2_expert_weights "
                         f"{tuple(fc2_expert_weights.shape)} must be ({G}, 2 I, {H}) and ({G}, {H}, I)")
    if H == 0 or H % 64 != 0 or I == 0 or I % 64 != 0:
        raise ValueError(f"hidden size {H} and intermediate size {I} must be positive multiples of 64 (pad them)")
    if not 1 <= G <= _MAX_EXPERTS:
        raise ValueError(f"{G} local experts: at most {_MAX_EXPERTS}")
    if token_selected_experts.dtype != torch.int32 or token_selected_experts.dim() != 2 \
            or token_selected_experts.shape[0] != T or not 1 <= token_selected_experts.shape[1] <= _MAX_TOP_K:
        raise ValueError(f"token_selected_experts must be int32 of shape ({T}, top_k <= {_MAX_TOP_K}), got "
                         f"{token_selected_experts.dtype} {tuple(token_selected_experts.shape)}")
    top_k = token_selected_experts.shape[1]
    if token_final_scales.dtype != torch.float32 or tuple(token_final_scales.shape) != (T, top_k):
        raise ValueError(f"token_final_scales must be float32 of shape ({T}, {top_k}), got {token_final_scales.dtype} "
                         f"{tuple(token_final_scales.shape)}")
    gates = [t for t in (swiglu_alpha, swiglu_beta, swiglu_limit) if t is not None]
    if gates and len(gates) != 3:
        raise ValueError("swiglu_alpha, swiglu_beta and swiglu_limit come all three or not at all")
    for name, t in (("swiglu_alpha", swiglu_alpha), ("swiglu_beta", swiglu_beta), ("swiglu_limit", swiglu_limit)):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (G,)):
            raise ValueError(f"{name} must be float32 of shape ({G},), got {t.dtype} {tuple(t.shape)}")
    if ep_size < 1 or not 0 <= ep_rank < ep_size or tp_size < 1 or not 0 <= tp_rank < tp_size:
        raise ValueError(f"ep_rank {ep_rank} / ep_size {ep_size} or tp_rank {tp_rank} / tp_size {tp_size} is not a rank of its size")
    if output is not None:
        _check_output_16bit(output, T, H, dtype)
    for name, t in (("fc1_expert_weights", fc1_expert_weights), ("fc2_expert_weights", fc2_expert_weights)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous: there is no silent copy of a weight tensor")
    for name, t in (("input", input), ("token_selected_experts", token_selected_experts),
                    ("token_final_scales", token_final_scales), ("fc1_expert_weights", fc1_expert_weights),
                    ("fc2_expert_weights", fc2_expert_weights), ("output", output)):
        if t is not None:
            _lib.require_gpu_tensor(t, name)
    if T == 0:
        return [output if output is not None else torch.empty((0, H), dtype=dtype, device=input.device)]

    # ---- the layer ----
    m_indptr, emap, p2e = moe_sort(token_selected_experts, ep_rank * G, G)
    act = moe_group_gemm_16bit(input, fc1_expert_weights, m_indptr, a_row_ids=p2e, swiglu=True, alpha=swiglu_alpha,
                               beta=swiglu_beta, limit=swiglu_limit, a_row_ids_div=top_k)
    gemm2_output = moe_group_gemm_16bit(act, fc2_expert_weights, m_indptr)
    return [moe_finalize_16bit(gemm2_output, token_final_scales, emap, output)]
