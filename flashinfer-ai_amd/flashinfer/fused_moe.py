"""Mixture-of-experts layer with MXFP8 activations and MXFP4 weights: ``trtllm_fp4_block_scale_moe`` and
``trtllm_fp4_block_scale_routed_moe`` of the reference's flashinfer/fused_moe/core.py (:1819-1948, :1951-2082) in their
MXFP8 x MXFP4 mode, ``RoutingMethodType`` (:62-76) and ``GatedActType`` (:164-168).

The layer is six steps on the device, in this order: route, permute, GEMM1, gated activation, GEMM2, finalize.
The GEMMs are ``group_gemm_mxfp8_mxfp4_nt_groupwise`` (csrc/gemm_mxfp4.hip); everything around them is csrc/moe.hip
behind fi_moe_* (include/fi_mi355.h).  The four stage functions ``moe_route``, ``moe_permute_mxfp8``,
``moe_gated_act_mxfp8`` and ``moe_finalize`` are this project's own (the reference runs the layer as one call; the
precedent is ``mxfp8_quantize_grouped``): the layer calls exactly them, so its result is bit for bit the result of
calling them one by one.

What differs from the reference: weights are plain ``[E_local, n, k / 2]`` MXFP4 with scales in the grouped
swizzled layout, as ``mxfp4_quantize_grouped`` returns them -- the trtllm-gen weight shuffle and gate / up row interleave
are NVIDIA kernel layouts and are neither applied nor accepted; rows ``[0, I)`` of GEMM1's output are the linear half and
rows ``[I, 2 I)`` the gate; GEMM1's output is rounded to bf16 before the activation.  Everything outside the mode above
(bf16 or nvfp4 activations, GeGlu, per-tensor output scales) raises NotImplementedError naming the argument, before
any launch.

Routing is every method of ``RoutingMethodType`` but ``Unspecified``.  ``DeepSeekV3`` (sigmoid scores, ``routing_bias``,
``topk_group`` of ``n_group`` expert groups by their top-2 sums, ``routed_scaling_factor``; without groups Kimi-K2's shape)
and ``Llama4`` (top-1, then sigmoid) run as one kernel of their own behind fi_moe_route_sigmoid; ``routing_bias``,
``n_group``, ``topk_group`` and a ``routed_scaling_factor`` other than 1 belong to ``DeepSeekV3`` and are refused with any
other method and in the routed call, where no routing runs.  An expert of a dropped group is never chosen, also
where the reference's kernel and the routine its tests compare it with would let it win against negative biased scores
(INTEGRATION.md).

``moe_permute_fp8_block`` and ``moe_gated_act_fp8_block`` (plain SwiGLU) are the same two stages on DeepSeek's fp8 block-scale
format, f32 scales per token and 128 columns instead of E8M0 bytes: with ``moe_route`` and ``moe_finalize`` they are the
steps of ``flashinfer.fused_moe_fp8.trtllm_fp8_block_scale_moe``, which lives in a module of its own.

Nothing here reads a device value on the host or synchronises, and every buffer's size depends on shapes alone, so a
call can be captured into a graph.
"""
from __future__ import annotations

import ctypes as C
from enum import IntEnum
from typing import List, Optional, Tuple

import torch

from . import _lib
from ._mx import BLOCK, contiguous_aligned, scale_bytes, sf_shape
from .gemm import _group_gemm_mxfp4_into

_MAX_EXPERTS = 512
_MAX_TOP_K = 8


# ref: flashinfer/fused_moe/core.py:62-76
class RoutingMethodType(IntEnum):
    # Default: Softmax -> TopK
    Default = 0
    # Renormalize: TopK -> Softmax
    Renormalize = 1
    # DeepSeekV3: Sigmoid -> RoutingBiasAdd -> Top2 in group -> Top4 groups -> Top8 experts from the Top4 groups
    DeepSeekV3 = 2
    # Llama4: Top1 -> Sigmoid
    Llama4 = 3
    # Qwen3: Softmax -> TopK -> Renormalize
    RenormalizeNaive = 4
    # TopK only (no softmax)
    TopK = 5
    # Unspecified
    Unspecified = 6


# ref: flashinfer/fused_moe/core.py:164-168
class GatedActType(IntEnum):
    SwiGlu = 0
    GeGlu = 1


_MAX_GROUPS = 64


def _check_no_deepseek_arguments(routing_bias, n_group, topk_group, routed_scaling_factor) -> None:
    """What only DeepSeekV3 routing takes, wherever that routing does not run."""
    if routing_bias is not None:
        raise NotImplementedError("routing_bias is not provided (it belongs to DeepSeekV3 routing): pass None")
    if n_group not in (None, 0) or topk_group not in (None, 0):
        raise NotImplementedError("n_group / topk_group (expert groups, DeepSeekV3 routing) are not provided: pass None")
    if routed_scaling_factor is not None and routed_scaling_factor != 1.0:
        raise NotImplementedError(f"routed_scaling_factor {routed_scaling_factor} is not provided: pass None or 1.0")


def _check_top_k(top_k: int, num_experts: int) -> None:
    if not 1 <= num_experts <= _MAX_EXPERTS:
        raise NotImplementedError(f"num_experts {num_experts} is not in [1, {_MAX_EXPERTS}]")
    if not 1 <= top_k <= min(_MAX_TOP_K, num_experts):
        raise NotImplementedError(f"top_k {top_k} is not in [1, min({_MAX_TOP_K}, num_experts = {num_experts})]")


def _check_routing(routing_method_type: int, top_k: int, num_experts: int, routing_bias: Optional[torch.Tensor],
                   n_group: Optional[int], topk_group: Optional[int],
                   routed_scaling_factor: Optional[float]) -> Tuple[int, int, int, float]:
    """The routing arguments of ``moe_route`` and the layer, without a tensor read: ``(method, n_group, topk_group,
    routed_scaling_factor)`` as the C ABI takes them, ``n_group`` 0 for no groups."""
    try:
        method = RoutingMethodType(int(routing_method_type))
    except ValueError:
        raise NotImplementedError(f"routing_method_type {routing_method_type} is not a routing method") from None
    if method == RoutingMethodType.Unspecified:
        raise NotImplementedError("routing_method_type Unspecified is not provided: name the method")
    if method == RoutingMethodType.DeepSeekV3 and routing_bias is None:
        raise NotImplementedError("routing_method_type DeepSeekV3 needs routing_bias: the bias is part of the method "
                                  "(pass zeros for none)")
    if method == RoutingMethodType.Llama4 and top_k != 1:
        raise NotImplementedError(f"routing_method_type Llama4 is top-1 routing: top_k {top_k} is not provided")
    _check_top_k(top_k, num_experts)
    if method != RoutingMethodType.DeepSeekV3:
        _check_no_deepseek_arguments(routing_bias, n_group, topk_group, routed_scaling_factor)
        return int(method), 0, 0, 1.0
    E = num_experts
    if routing_bias.dtype not in (torch.float32, torch.bfloat16) or tuple(routing_bias.shape) != (E,):
        raise ValueError(f"routing_bias must be float32 or bfloat16 of shape ({E},), got {routing_bias.dtype} "
                         f"{tuple(routing_bias.shape)}")
    n_group, topk_group = int(n_group or 0), int(topk_group or 0)
    if n_group < 0 or topk_group < 0:
        raise ValueError(f"n_group {n_group} and topk_group {topk_group} must not be negative")
    if n_group <= 1:
        if topk_group > n_group:
            raise ValueError(f"topk_group {topk_group} is given without expert groups (n_group {n_group})")
        n_group = topk_group = 0
    else:
        if n_group > _MAX_GROUPS:
            raise NotImplementedError(f"n_group {n_group} is not in [0, {_MAX_GROUPS}]")
        if E % n_group != 0:
            raise ValueError(f"num_experts {E} is not a multiple of n_group {n_group}")
        epg = E // n_group
        if epg < 2:
            raise NotImplementedError(f"n_group {n_group} leaves {epg} expert per group: a group's score is the sum of two")
        if not 1 <= topk_group <= n_group:
            raise ValueError(f"topk_group {topk_group} is not in [1, n_group = {n_group}]")
        if top_k > topk_group * epg:
            raise ValueError(f"top_k {top_k} exceeds the {topk_group * epg} experts of topk_group {topk_group} groups of {epg}")
    return int(method), n_group, topk_group, 1.0 if routed_scaling_factor is None else float(routed_scaling_factor)


def moe_route(routing_logits: torch.Tensor, top_k: int, routing_method_type: int = RoutingMethodType.Default,
              routing_bias: Optional[torch.Tensor] = None, n_group: Optional[int] = None,
              topk_group: Optional[int] = None,
              routed_scaling_factor: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Router logits -> expert ids and weights.  Not part of the reference, which routes inside its fused call.

    ``routing_logits`` is f32 or bf16 ``[T, E]`` with ``E <= 512`` and ``1 <= top_k <= min(8, E)``.  Returns ``(ids, weights)``:
    int32 and bf16 ``[T, top_k]``.  The weights are computed in f32 and rounded once; a NaN logit counts as -inf.

    ``Default``, ``Renormalize``, ``RenormalizeNaive``, ``TopK``: slot ``j`` of a token is the expert of its ``j``-th largest
    logit, ties to the lower expert index.  ``Default`` softmax over all experts; ``Renormalize`` softmax over the chosen
    logits; ``RenormalizeNaive`` the ``Default`` weights divided by their sum; ``TopK`` the logits themselves.  The four
    trailing arguments belong to ``DeepSeekV3`` and are refused.

    ``DeepSeekV3`` (``routing_bias`` f32 or bf16 ``[E]`` is required): ``s = sigmoid(logit)``, ``b = s + routing_bias``.  With
    ``n_group > 1`` the experts ``[g * epg, (g + 1) * epg)``, ``epg = E / n_group``, are group ``g``; a group's score is the sum
    of its two largest ``b`` and only the ``topk_group`` groups of the largest score (ties to the lower group) stay
    candidates: ``E % n_group == 0``, ``epg >= 2``, ``n_group <= 64``, ``1 <= topk_group <= n_group``, ``top_k <= topk_group *
    epg``.  With ``n_group`` ``None``, 0 or 1 every expert is a candidate.  Slot ``j`` is the candidate of the ``j``-th largest
    ``b``, ties to the lower expert, and ``w[j] = s[id_j] * routed_scaling_factor / (sum_j s[id_j] + 1e-20)``;
    ``routed_scaling_factor=None`` is 1.  An expert of a dropped group is never chosen, also when every kept ``b`` is
    negative.

    ``Llama4``: ``top_k == 1``; the expert of the largest logit, ties to the lower index, with weight ``sigmoid(logit)``.
    """
    if routing_logits.dim() != 2:
        raise ValueError(f"routing_logits must be 2D (T, E), got shape {tuple(routing_logits.shape)}")
    T, E = routing_logits.shape
    method, n_group, topk_group, scale = _check_routing(routing_method_type, top_k, E, routing_bias, n_group, topk_group,
                                                        routed_scaling_factor)
    if routing_logits.dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError(f"routing_logits has dtype {routing_logits.dtype}: only float32 and bfloat16")
    _lib.require_gpu_tensor(routing_logits, "routing_logits")
    if routing_bias is not None:
        _lib.require_gpu_tensor(routing_bias, "routing_bias")
        if routing_bias.device != routing_logits.device:
            raise ValueError(f"routing_bias is on {routing_bias.device}, routing_logits on {routing_logits.device}")
    ids = torch.empty((T, top_k), dtype=torch.int32, device=routing_logits.device)
    weights = torch.empty((T, top_k), dtype=torch.bfloat16, device=routing_logits.device)
    if T == 0:
        return ids, weights
    logits = routing_logits.contiguous()
    with torch.cuda.device(logits.device):
        if method in (RoutingMethodType.DeepSeekV3, RoutingMethodType.Llama4):
            bias = None if routing_bias is None else routing_bias.contiguous()
            p = _lib.fi_moe_route_sigmoid_params_t(
                logits=logits.data_ptr(), bias=_lib.ptr(bias), topk_ids=ids.data_ptr(), topk_weights=weights.data_ptr(),
                num_tokens=T, num_experts=E, top_k=top_k, n_group=n_group, topk_group=topk_group,
                routed_scaling_factor=scale, method=method, dtype=_lib.fi_dtype(logits.dtype),
                bias_dtype=_lib.fi_dtype(torch.float32 if bias is None else bias.dtype))
            _lib.check(_lib.lib().fi_moe_route_sigmoid(C.byref(p), _lib.current_stream(logits.device)), "moe_route_sigmoid")
        else:
            p = _lib.fi_moe_route_params_t(
                logits=logits.data_ptr(), topk_ids=ids.data_ptr(), topk_weights=weights.data_ptr(), num_tokens=T,
                num_experts=E, top_k=top_k, method=method, dtype=_lib.fi_dtype(logits.dtype))
            _lib.check(_lib.lib().fi_moe_route(C.byref(p), _lib.current_stream(logits.device)), "moe_route")
    return ids, weights


def _check_activations(hidden_states: torch.Tensor, hidden_states_scale: Optional[torch.Tensor]) -> None:
    if hidden_states.dtype == torch.bfloat16:
        raise NotImplementedError(
            "hidden_states in bfloat16 is not provided: quantise with flashinfer.mxfp8_quantize(x, False) and pass "
            "float8_e4m3fn hidden_states with their hidden_states_scale")
    if hidden_states.dtype != torch.float8_e4m3fn:
        raise NotImplementedError(
            f"hidden_states has dtype {hidden_states.dtype}: only MXFP8 (float8_e4m3fn) activations, not nvfp4")
    if hidden_states_scale is None:
        raise NotImplementedError("hidden_states_scale is None: MXFP8 hidden_states carry one E8M0 byte per 32 elements")
    if hidden_states_scale.dtype not in (torch.uint8, torch.float8_e4m3fn):
        raise NotImplementedError(
            f"hidden_states_scale has dtype {hidden_states_scale.dtype}: E8M0 bytes as uint8 or float8_e4m3fn")
    if hidden_states.dim() != 2:
        raise ValueError(f"hidden_states must be 2D (T, H), got shape {tuple(hidden_states.shape)}")
    T, H = hidden_states.shape
    if H == 0 or H % 128 != 0:
        raise NotImplementedError(f"hidden_states has hidden size {H}: it must be a multiple of 128 (pad it)")
    if hidden_states_scale.numel() != T * (H // BLOCK):
        raise ValueError(f"hidden_states_scale holds {hidden_states_scale.numel()} bytes, {T * (H // BLOCK)} needed "
                         "(linear layout, one byte per 32 elements)")


def _permute_into(topk_ids: torch.Tensor, hidden_states: torch.Tensor, hidden_states_scale: torch.Tensor,
                  local_expert_offset: int, local_num_experts: int, packed: bool, m_indptr: torch.Tensor,
                  emap: torch.Tensor, x_permuted: torch.Tensor, sf_permuted: torch.Tensor,
                  weights: Optional[torch.Tensor]) -> None:
    """fi_moe_permute_mxfp8 on checked tensors (T > 0) into pre-allocated outputs; every byte of ``sf_permuted`` is
    written.  The workspace (block histograms and the inverse map) is sized by shapes alone."""
    T, top_k = topk_ids.shape
    n, G, dev = T * top_k, local_num_experts, hidden_states.device
    blocks = -(-n // _lib.FI_MOE_SORT_BLOCK)
    workspace = torch.empty((blocks * G + n,), dtype=torch.int32, device=dev)
    ids, x = topk_ids.contiguous(), contiguous_aligned(hidden_states, 16)
    x_sf = contiguous_aligned(scale_bytes(hidden_states_scale), 4)
    p = _lib.fi_moe_permute_params_t(
        topk_ids=ids.data_ptr(), x=x.data_ptr(), x_sf=x_sf.data_ptr(), m_indptr=m_indptr.data_ptr(),
        expanded_to_permuted=emap.data_ptr(), x_permuted=x_permuted.data_ptr(), sf_permuted=sf_permuted.data_ptr(),
        unpacked_weights=_lib.ptr(weights), workspace=workspace.data_ptr(), sf_bytes=sf_permuted.numel(),
        workspace_bytes=_lib.nbytes(workspace), num_tokens=T, top_k=top_k, hidden=hidden_states.shape[1],
        local_expert_offset=local_expert_offset, local_num_experts=G, packed=int(bool(packed)))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().fi_moe_permute_mxfp8(C.byref(p), _lib.current_stream(dev)), "moe_permute_mxfp8")


def moe_permute_mxfp8(
    topk_ids: torch.Tensor,
    hidden_states: torch.Tensor,
    hidden_states_scale: torch.Tensor,
    local_expert_offset: int,
    local_num_experts: int,
    packed: bool = False,
) -> Tuple[torch.Tensor, ...]:
    """Sort the slots by local expert and gather the MXFP8 rows into the row operand of GEMM1.  Not part of the reference.

    ``topk_ids`` is int32 ``[T, top_k]``: expert ids, or with ``packed`` the routed call's packing (low 16 bits the expert,
    high 16 bits the bf16 weight).  ``hidden_states`` float8_e4m3fn ``[T, H]`` and ``hidden_states_scale`` ``T * H / 32`` E8M0
    bytes in the linear layout, as ``mxfp8_quantize(x, False)`` returns them.  Returns ``(m_indptr, expanded_idx_to_permuted_idx,
    x_permuted, sf_permuted)`` and with ``packed`` a fifth tensor, the bf16 weights ``[T, top_k]``:

    * ``m_indptr`` int32 ``[local_num_experts + 1]``: the row segments of the local experts;
    * ``expanded_idx_to_permuted_idx`` int32 ``[T * top_k]``: the row of slot ``t * top_k + j``, -1 for a non-local expert;
    * ``x_permuted`` float8_e4m3fn ``[T * top_k, H]``; rows at or past ``m_indptr[-1]`` are unwritten;
    * ``sf_permuted`` uint8 ``[sf_row_offset(T * top_k, local_num_experts), H / 32]``, grouped swizzled, padding 0.

    Within an expert the rows ascend by expanded index; experts follow one another without padding rows.
    """
    if topk_ids.dtype != torch.int32 or topk_ids.dim() != 2:
        raise ValueError("topk_ids must be a 2D int32 tensor (T, top_k)")
    _check_activations(hidden_states, hidden_states_scale)
    T, top_k = topk_ids.shape
    H = hidden_states.shape[1]
    if hidden_states.shape[0] != T:
        raise ValueError(f"topk_ids has {T} rows, hidden_states {hidden_states.shape[0]}")
    if not 1 <= top_k <= _MAX_TOP_K:
        raise NotImplementedError(f"top_k {top_k} is not in [1, {_MAX_TOP_K}]")
    if not 1 <= local_num_experts <= _MAX_EXPERTS or local_expert_offset < 0:
        raise NotImplementedError(
            f"local_num_experts {local_num_experts} is not in [1, {_MAX_EXPERTS}] or local_expert_offset {local_expert_offset} < 0")
    for t, name in ((topk_ids, "topk_ids"), (hidden_states, "hidden_states"), (hidden_states_scale, "hidden_states_scale")):
        _lib.require_gpu_tensor(t, name)
    dev = hidden_states.device
    n, G = T * top_k, local_num_experts
    m_indptr = torch.empty((G + 1,), dtype=torch.int32, device=dev)
    emap = torch.empty((n,), dtype=torch.int32, device=dev)
    x_permuted = torch.empty((n, H), dtype=torch.float8_e4m3fn, device=dev)
    sf_permuted = torch.empty(sf_shape(n, H // BLOCK, groups=G) if n else (0, H // BLOCK), dtype=torch.uint8, device=dev)
    weights = torch.empty((T, top_k), dtype=torch.bfloat16, device=dev) if packed else None
    if T == 0:
        m_indptr.zero_()
    else:
        _permute_into(topk_ids, hidden_states, hidden_states_scale, local_expert_offset, G, packed, m_indptr, emap,
                      x_permuted, sf_permuted, weights)
    if packed:
        return m_indptr, emap, x_permuted, sf_permuted, weights
    return m_indptr, emap, x_permuted, sf_permuted


def _per_expert(t: Optional[torch.Tensor], name: str, shape: Tuple[int, ...]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32 or tuple(t.shape) != shape:
        raise ValueError(f"{name} must be float32 of shape {shape}, got {t.dtype} {tuple(t.shape)}")
    _lib.require_gpu_tensor(t, name)
    return t


def _gated_act_into(gemm1_output: torch.Tensor, m_indptr: torch.Tensor, bias: Optional[torch.Tensor],
                    alpha: Optional[torch.Tensor], beta: Optional[torch.Tensor], limit: Optional[torch.Tensor],
                    q: torch.Tensor, sf: torch.Tensor) -> None:
    """fi_moe_gated_act_mxfp8 on checked tensors (cum_m > 0) into pre-allocated outputs; every byte of ``sf`` is written,
    rows of ``q`` at or past ``m_indptr[-1]`` are not."""
    cum_m, two_i = gemm1_output.shape
    dev = gemm1_output.device
    x = contiguous_aligned(gemm1_output, 16)
    p = _lib.fi_moe_gated_act_params_t(
        x=x.data_ptr(), m_indptr=m_indptr.contiguous().data_ptr(), bias=_lib.ptr(bias), alpha=_lib.ptr(alpha),
        beta=_lib.ptr(beta), limit=_lib.ptr(limit), q=q.data_ptr(), sf=sf.data_ptr(), sf_bytes=sf.numel(), cum_m=cum_m,
        intermediate=two_i // 2, num_groups=m_indptr.shape[0] - 1)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().fi_moe_gated_act_mxfp8(C.byref(p), _lib.current_stream(dev)), "moe_gated_act_mxfp8")


def moe_gated_act_mxfp8(
    gemm1_output: torch.Tensor,
    m_indptr: torch.Tensor,
    gemm1_bias: Optional[torch.Tensor] = None,
    gemm1_alpha: Optional[torch.Tensor] = None,
    gemm1_beta: Optional[torch.Tensor] = None,
    gemm1_clamp_limit: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """The gated activation between the two GEMMs, quantised to MXFP8 for the second.  Not part of the reference.

    ``gemm1_output`` is bf16 ``[cum_m, 2 I]`` with ``I % 128 == 0``: columns ``[0, I)`` the linear half ``x1``, ``[I, 2 I)`` the
    gate ``x2``.  For a row of expert ``g``, in f32 (ref: tests/moe/test_trtllm_cutlass_fused_moe.py:195-203)::

        gt = min(x2 + bias[g, I:], limit[g]);  l = clamp(x1 + bias[g, :I], -limit[g], limit[g]) + beta[g]
        act = gt * sigmoid(alpha[g] * gt) * l

    ``gemm1_bias`` f32 ``[G, 2 I]``, the others f32 ``[G]``; ``None`` means bias 0, alpha 1, beta 0, limit +inf.  Returns
    ``(q, sf)``: float8_e4m3fn ``[cum_m, I]`` and uint8 ``[sf_row_offset(cum_m, G), I / 32]`` grouped swizzled with padding 0,
    by the rule of ``mxfp8_quantize``.  Rows at or past ``m_indptr[-1]`` are not written.
    """
    if gemm1_output.dtype != torch.bfloat16 or gemm1_output.dim() != 2:
        raise ValueError("gemm1_output must be a 2D bfloat16 tensor (cum_m, 2 I)")
    if m_indptr.dtype != torch.int32 or m_indptr.dim() != 1 or m_indptr.shape[0] < 2:
        raise ValueError("m_indptr must be a 1D int32 tensor of G + 1 >= 2 entries")
    cum_m, two_i = gemm1_output.shape
    I, G = two_i // 2, m_indptr.shape[0] - 1
    if two_i == 0 or two_i % 256 != 0:
        raise NotImplementedError(f"intermediate_size {two_i / 2:g} must be a multiple of 128")
    if G > _MAX_EXPERTS:
        raise NotImplementedError(f"{G} groups: at most {_MAX_EXPERTS}")
    _lib.require_gpu_tensor(gemm1_output, "gemm1_output")
    _lib.require_gpu_tensor(m_indptr, "m_indptr")
    bias = _per_expert(gemm1_bias, "gemm1_bias", (G, two_i))
    bias = None if bias is None else contiguous_aligned(bias, 16)
    alpha, beta, limit = (
        None if t is None else t.contiguous() for t in (
            _per_expert(gemm1_alpha, "gemm1_alpha", (G,)),
            _per_expert(gemm1_beta, "gemm1_beta", (G,)),
            _per_expert(gemm1_clamp_limit, "gemm1_clamp_limit", (G,))))
    dev = gemm1_output.device
    q = torch.empty((cum_m, I), dtype=torch.float8_e4m3fn, device=dev)
    sf = torch.empty(sf_shape(cum_m, I // BLOCK, groups=G) if cum_m else (0, I // BLOCK), dtype=torch.uint8, device=dev)
    if cum_m == 0:
        return q, sf
    _gated_act_into(gemm1_output, m_indptr, bias, alpha, beta, limit, q, sf)
    return q, sf


def moe_finalize(
    gemm2_output: torch.Tensor,
    expert_weights: torch.Tensor,
    expanded_idx_to_permuted_idx: torch.Tensor,
    gemm2_bias: Optional[torch.Tensor] = None,
    m_indptr: Optional[torch.Tensor] = None,
    output: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """``out[t] = bf16(sum_j w[t, j] * (y[p(t, j)] + bias[g(t, j)]))`` over the slots with ``p >= 0``, accumulated in f32 in
    the order of ``j``; a token without a local slot gets zeros.  Not part of the reference.

    ``gemm2_output`` bf16 ``[T * top_k, H]``, ``expert_weights`` bf16 ``[T, top_k]``, ``expanded_idx_to_permuted_idx`` int32
    ``[T * top_k]`` -- the triple of ``do_finalize=False``.  ``gemm2_bias`` f32 ``[G, H]`` needs ``m_indptr`` (``[G + 1]``), which
    tells the expert of a row.  ``output``, if given, is a contiguous bf16 ``[T, H]`` tensor and is returned.
    """
    if gemm2_output.dtype != torch.bfloat16 or gemm2_output.dim() != 2:
        raise ValueError("gemm2_output must be a 2D bfloat16 tensor (T * top_k, H)")
    if expert_weights.dtype != torch.bfloat16 or expert_weights.dim() != 2:
        raise ValueError("expert_weights must be a 2D bfloat16 tensor (T, top_k)")
    T, top_k = expert_weights.shape
    rows, H = gemm2_output.shape
    if expanded_idx_to_permuted_idx.dtype != torch.int32 or expanded_idx_to_permuted_idx.numel() != T * top_k:
        raise ValueError(f"expanded_idx_to_permuted_idx must be int32 with {T * top_k} entries")
    if not 1 <= top_k <= _MAX_TOP_K:
        raise NotImplementedError(f"top_k {top_k} is not in [1, {_MAX_TOP_K}]")
    if H == 0 or H % 8 != 0:
        raise NotImplementedError(f"hidden size {H} must be a multiple of 8")
    G = 0
    if gemm2_bias is not None:
        if m_indptr is None or m_indptr.dtype != torch.int32 or m_indptr.dim() != 1 or m_indptr.shape[0] < 2:
            raise ValueError("gemm2_bias needs m_indptr, a 1D int32 tensor of G + 1 >= 2 entries")
        G = m_indptr.shape[0] - 1
        _lib.require_gpu_tensor(m_indptr, "m_indptr")
    bias = _per_expert(gemm2_bias, "gemm2_bias", (G, H))
    bias = None if bias is None else contiguous_aligned(bias, 16)
    for t, name in ((gemm2_output, "gemm2_output"), (expert_weights, "expert_weights"),
                    (expanded_idx_to_permuted_idx, "expanded_idx_to_permuted_idx")):
        _lib.require_gpu_tensor(t, name)
    dev = gemm2_output.device
    if output is None:
        output = torch.empty((T, H), dtype=torch.bfloat16, device=dev)
    else:
        _check_output(output, T, H)
        _lib.require_gpu_tensor(output, "output")
    if T == 0:
        return output
    y = contiguous_aligned(gemm2_output, 16)
    p = _lib.fi_moe_finalize_params_t(
        y=y.data_ptr(), weights=expert_weights.contiguous().data_ptr(),
        expanded_to_permuted=expanded_idx_to_permuted_idx.contiguous().data_ptr(), bias=_lib.ptr(bias),
        m_indptr=_lib.ptr(m_indptr.contiguous() if bias is not None else None), out=output.data_ptr(), num_tokens=T,
        top_k=top_k, hidden=H, num_groups=G, rows=rows)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().fi_moe_finalize(C.byref(p), _lib.current_stream(dev)), "moe_finalize")
    return output


def _check_output(output: torch.Tensor, T: int, H: int) -> None:
    if output.dtype != torch.bfloat16 or tuple(output.shape) != (T, H) or not output.is_contiguous() \
            or output.data_ptr() % 16 != 0:
        raise ValueError(f"output must be a contiguous, 16-byte aligned bfloat16 tensor of shape ({T}, {H})")


def _check_weights(name: str, w: torch.Tensor, sf: torch.Tensor, G: int, n: int, k: int) -> None:
    if w.dtype != torch.uint8 or tuple(w.shape) != (G, n, k // 2):
        raise NotImplementedError(
            f"{name} must be uint8 of shape ({G}, {n}, {k // 2}) (plain MXFP4, two e2m1 codes per byte, not shuffled), got "
            f"{w.dtype} {tuple(w.shape)}")
    n_pad, nkb = sf_shape(n, k // BLOCK)
    if sf.dtype != torch.uint8 or sf.numel() != G * n_pad * nkb:
        raise NotImplementedError(
            f"{name}_scale must be uint8 with {G * n_pad * nkb} bytes in the grouped swizzled layout, as "
            f"mxfp4_quantize_grouped returns it, got {sf.dtype} with {sf.numel()}")


def _moe(routing_logits, topk_ids, routing_bias, hidden_states, hidden_states_scale, gemm1_weights, gemm1_weights_scale,
         gemm1_bias, gemm1_alpha, gemm1_beta, gemm1_clamp_limit, gemm2_weights, gemm2_weights_scale, gemm2_bias,
         output1_scale_scalar, output1_scale_gate_scalar, output2_scale_scalar, num_experts, top_k, n_group, topk_group,
         intermediate_size, local_expert_offset, local_num_experts, routed_scaling_factor, tile_tokens_dim,
         routing_method_type, do_finalize, enable_pdl, gated_act_type, output, tune_max_num_tokens) -> List[torch.Tensor]:
    # ---- what is not provided, before anything touches the device ----
    if topk_ids is None:
        _check_routing(routing_method_type, top_k, num_experts, routing_bias, n_group, topk_group, routed_scaling_factor)
    else:  # no routing runs
        _check_no_deepseek_arguments(routing_bias, n_group, topk_group, routed_scaling_factor)
    for name, t in (("output1_scale_scalar", output1_scale_scalar), ("output1_scale_gate_scalar", output1_scale_gate_scalar),
                    ("output2_scale_scalar", output2_scale_scalar)):
        if t is not None:
            raise NotImplementedError(f"{name} must be None: MX operands carry their own scales")
    if int(gated_act_type) != GatedActType.SwiGlu:
        raise NotImplementedError(f"gated_act_type {gated_act_type} is not provided: only SwiGlu (0)")
    _check_top_k(top_k, num_experts)
    _check_activations(hidden_states, hidden_states_scale)
    T, H = hidden_states.shape
    I, G = intermediate_size, local_num_experts
    if I <= 0 or I % 128 != 0:
        raise NotImplementedError(f"intermediate_size {I} must be a multiple of 128 (pad it)")
    if local_expert_offset < 0 or G < 1 or local_expert_offset + G > num_experts:
        raise ValueError(f"the local experts [{local_expert_offset}, {local_expert_offset + G}) are not within "
                         f"[0, num_experts = {num_experts})")
    _check_weights("gemm1_weights", gemm1_weights, gemm1_weights_scale, G, 2 * I, H)
    _check_weights("gemm2_weights", gemm2_weights, gemm2_weights_scale, G, H, I)
    _per_expert(gemm1_bias, "gemm1_bias", (G, 2 * I))
    _per_expert(gemm1_alpha, "gemm1_alpha", (G,))
    _per_expert(gemm1_beta, "gemm1_beta", (G,))
    _per_expert(gemm1_clamp_limit, "gemm1_clamp_limit", (G,))
    _per_expert(gemm2_bias, "gemm2_bias", (G, H))
    # tile_tokens_dim, tune_max_num_tokens and enable_pdl tune NVIDIA kernels; the reference's Python does not validate
    # them either
    if gemm2_bias is not None and not do_finalize:
        raise NotImplementedError("gemm2_bias with do_finalize=False is not provided: the bias is added by the finalize "
                                  "step (moe_finalize takes it)")
    if topk_ids is None:
        if routing_logits.dim() != 2 or tuple(routing_logits.shape) != (T, num_experts):
            raise ValueError(f"routing_logits must have shape ({T}, {num_experts}), got {tuple(routing_logits.shape)}")
        if routing_logits.dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError(f"routing_logits has dtype {routing_logits.dtype}: only float32 and bfloat16")
    elif topk_ids.dtype != torch.int32 or tuple(topk_ids.shape) != (T, top_k):
        raise ValueError(f"topk_ids must be int32 of shape ({T}, {top_k}), got {topk_ids.dtype} {tuple(topk_ids.shape)}")
    if output is not None:
        _check_output(output, T, H)
    tensors = [("routing_logits", routing_logits), ("routing_bias", routing_bias), ("topk_ids", topk_ids),
               ("hidden_states", hidden_states),
               ("hidden_states_scale", hidden_states_scale), ("gemm1_weights", gemm1_weights),
               ("gemm1_weights_scale", gemm1_weights_scale), ("gemm2_weights", gemm2_weights),
               ("gemm2_weights_scale", gemm2_weights_scale), ("output", output)]
    for name, t in tensors:
        if t is not None:
            _lib.require_gpu_tensor(t, name)
    dev = hidden_states.device
    if T == 0:
        empty = torch.empty((0, H), dtype=torch.bfloat16, device=dev)
        if do_finalize:
            return [output if output is not None else empty]
        return [empty, torch.empty((0, top_k), dtype=torch.bfloat16, device=dev),
                torch.empty((0,), dtype=torch.int32, device=dev)]

    # ---- the layer ----
    if topk_ids is None:
        ids, expert_weights = moe_route(routing_logits, top_k, routing_method_type, routing_bias=routing_bias,
                                        n_group=n_group, topk_group=topk_group, routed_scaling_factor=routed_scaling_factor)
        m_indptr, emap, x_perm, sf_perm = moe_permute_mxfp8(ids, hidden_states, hidden_states_scale, local_expert_offset, G)
    else:
        m_indptr, emap, x_perm, sf_perm, expert_weights = moe_permute_mxfp8(
            topk_ids, hidden_states, hidden_states_scale, local_expert_offset, G, packed=True)
    n = T * top_k
    gemm1_output = torch.empty((n, 2 * I), dtype=torch.bfloat16, device=dev)
    _group_gemm_mxfp4_into(x_perm, gemm1_weights, sf_perm, gemm1_weights_scale, gemm1_output, m_indptr, 2 * I, H)
    act, act_sf = moe_gated_act_mxfp8(gemm1_output, m_indptr, gemm1_bias, gemm1_alpha, gemm1_beta, gemm1_clamp_limit)
    gemm2_output = torch.empty((n, H), dtype=torch.bfloat16, device=dev)
    _group_gemm_mxfp4_into(act, gemm2_weights, act_sf, gemm2_weights_scale, gemm2_output, m_indptr, H, I)
    if not do_finalize:
        return [gemm2_output, expert_weights, emap]
    return [moe_finalize(gemm2_output, expert_weights, emap, gemm2_bias, m_indptr, output)]


def trtllm_fp4_block_scale_moe(
    routing_logits: torch.Tensor,
    routing_bias: Optional[torch.Tensor],
    hidden_states: torch.Tensor,
    hidden_states_scale: Optional[torch.Tensor],
    gemm1_weights: torch.Tensor,
    gemm1_weights_scale: torch.Tensor,
    gemm1_bias: Optional[torch.Tensor],
    gemm1_alpha: Optional[torch.Tensor],
    gemm1_beta: Optional[torch.Tensor],
    gemm1_clamp_limit: Optional[torch.Tensor],
    gemm2_weights: torch.Tensor,
    gemm2_weights_scale: torch.Tensor,
    gemm2_bias: Optional[torch.Tensor],
    output1_scale_scalar: Optional[torch.Tensor],
    output1_scale_gate_scalar: Optional[torch.Tensor],
    output2_scale_scalar: Optional[torch.Tensor],
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
    do_finalize: bool = True,
    enable_pdl: Optional[bool] = None,
    gated_act_type: int = 0,
    output: Optional[torch.Tensor] = None,
    tune_max_num_tokens: int = 8192,
) -> List[torch.Tensor]:
    """MoE layer with MXFP8 activations and MXFP4 weights (ref: flashinfer/fused_moe/core.py:1819-1948).

    routing_logits : ``[T, num_experts]`` f32 / bf16, ``num_experts <= 512``, ``1 <= top_k <= min(8, num_experts)``.
    hidden_states, hidden_states_scale : float8_e4m3fn ``[T, H]`` and ``T * H / 32`` E8M0 bytes (uint8 or float8_e4m3fn),
        linear layout -- ``mxfp8_quantize(x, False)``.  ``H % 128 == 0``.
    gemm1_weights, gemm1_weights_scale : uint8 ``[E_local, 2 I, H / 2]`` and its grouped swizzled scales, as
        ``mxfp4_quantize_grouped`` returns them; rows ``[0, I)`` produce the linear half, ``[I, 2 I)`` the gate.
    gemm1_bias, gemm1_alpha, gemm1_beta, gemm1_clamp_limit : f32 ``[E_local, 2 I]`` / ``[E_local]`` or None (see
        ``moe_gated_act_mxfp8``).
    gemm2_weights, gemm2_weights_scale : uint8 ``[E_local, H, I / 2]`` and scales; gemm2_bias f32 ``[E_local, H]`` or None.
    routing_method_type : any but Unspecified (see ``moe_route``).  gated_act_type : SwiGlu.
    routing_bias, n_group, topk_group, routed_scaling_factor : with DeepSeekV3, ``routing_bias`` f32 / bf16
        ``[num_experts]`` (required), ``topk_group`` of ``n_group`` expert groups (``n_group`` None, 0 or 1: none) and the
        factor on the weights (None: 1); with any other method None, the factor None or 1.0.  Llama4 takes ``top_k`` 1.
    output1_scale_scalar, output1_scale_gate_scalar, output2_scale_scalar : None.
    tile_tokens_dim, tune_max_num_tokens, enable_pdl : validated, then ignored.
    output : optional contiguous bf16 ``[T, H]``.

    Returns ``[out]`` (bf16 ``[T, H]``) with ``do_finalize``, else ``[gemm2_output, expert_weights,
    expanded_idx_to_permuted_idx]``: bf16 ``[T * top_k, H]`` (rows past the local count unwritten), bf16 ``[T, top_k]``,
    int32 ``[T * top_k]`` (-1 for a slot on a non-local expert; ``moe_finalize`` turns the triple into ``out``).
    """
    return _moe(routing_logits, None, routing_bias, hidden_states, hidden_states_scale, gemm1_weights, gemm1_weights_scale,
                gemm1_bias, gemm1_alpha, gemm1_beta, gemm1_clamp_limit, gemm2_weights, gemm2_weights_scale, gemm2_bias,
                output1_scale_scalar, output1_scale_gate_scalar, output2_scale_scalar, num_experts, top_k, n_group,
                topk_group, intermediate_size, local_expert_offset, local_num_experts, routed_scaling_factor,
                tile_tokens_dim, routing_method_type, do_finalize, enable_pdl, gated_act_type, output, tune_max_num_tokens)


def trtllm_fp4_block_scale_routed_moe(
    topk_ids: torch.Tensor,
    routing_bias: Optional[torch.Tensor],
    hidden_states: torch.Tensor,
    hidden_states_scale: Optional[torch.Tensor],
    gemm1_weights: torch.Tensor,
    gemm1_weights_scale: torch.Tensor,
    gemm1_bias: Optional[torch.Tensor],
    gemm1_alpha: Optional[torch.Tensor],
    gemm1_beta: Optional[torch.Tensor],
    gemm1_clamp_limit: Optional[torch.Tensor],
    gemm2_weights: torch.Tensor,
    gemm2_weights_scale: torch.Tensor,
    gemm2_bias: Optional[torch.Tensor],
    output1_scale_scalar: Optional[torch.Tensor],
    output1_scale_gate_scalar: Optional[torch.Tensor],
    output2_scale_scalar: Optional[torch.Tensor],
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
    do_finalize: bool = True,
    enable_pdl: Optional[bool] = None,
    gated_act_type: int = 0,
    output: Optional[torch.Tensor] = None,
    tune_max_num_tokens: int = 8192,
) -> List[torch.Tensor]:
    """``trtllm_fp4_block_scale_moe`` on experts chosen by the caller (ref: flashinfer/fused_moe/core.py:1951-2082).

    topk_ids : int32 ``[T, top_k]``; the low 16 bits of an entry are the unsigned expert index, the high 16 bits the bit
    pattern of the bf16 weight.  No routing kernel runs and ``routing_method_type`` is not used: ``routing_bias``, ``n_group``
    and ``topk_group`` are None and ``routed_scaling_factor`` None or 1.0.  Everything else as ``trtllm_fp4_block_scale_moe``.
    """
    return _moe(None, topk_ids, routing_bias, hidden_states, hidden_states_scale, gemm1_weights, gemm1_weights_scale,
                gemm1_bias, gemm1_alpha, gemm1_beta, gemm1_clamp_limit, gemm2_weights, gemm2_weights_scale, gemm2_bias,
                output1_scale_scalar, output1_scale_gate_scalar, output2_scale_scalar, num_experts, top_k, n_group,
                topk_group, intermediate_size, local_expert_offset, local_num_experts, routed_scaling_factor,
                tile_tokens_dim, routing_method_type, do_finalize, enable_pdl, gated_act_type, output, tune_max_num_tokens)


# ---- the fp8 block-scale layer (DeepSeek-V3 / R1 checkpoints) -----------------------------------------------------------
_FP8_BLOCK = 128


def _check_fp8_block_activations(hidden_states: torch.Tensor, hidden_states_scale: torch.Tensor) -> None:
    if hidden_states.dtype != torch.float8_e4m3fn:
        raise NotImplementedError(
            f"hidden_states has dtype {hidden_states.dtype}: only float8_e4m3fn with float32 hidden_states_scale "
            "(flashinfer.fp8_quantization.fp8_quantize_1x128 makes both)")
    if hidden_states.dim() != 2:
        raise ValueError(f"hidden_states must be 2D (T, H), got shape {tuple(hidden_states.shape)}")
    T, H = hidden_states.shape
    if H == 0 or H % _FP8_BLOCK != 0:
        raise NotImplementedError(f"hidden_states has hidden size {H}: it must be a multiple of 128 (pad it)")
    if hidden_states_scale is None or hidden_states_scale.dtype != torch.float32:
        raise NotImplementedError("hidden_states_scale must be a float32 tensor: one scale per token and 128 columns")
    if tuple(hidden_states_scale.shape) != (H // _FP8_BLOCK, T):
        raise ValueError(f"hidden_states_scale must have shape ({H // _FP8_BLOCK}, {T}) = (H / 128, T) with any strides, got "
                         f"{tuple(hidden_states_scale.shape)}")


def _permute_fp8_block_into(topk_ids: torch.Tensor, hidden_states: torch.Tensor, hidden_states_scale: torch.Tensor,
                            local_expert_offset: int, local_num_experts: int, packed: bool, m_indptr: torch.Tensor,
                            emap: torch.Tensor, x_permuted: torch.Tensor, scale_permuted: torch.Tensor,
                            weights: Optional[torch.Tensor]) -> None:
    """fi_moe_permute_fp8_block on checked tensors (T > 0) into pre-allocated outputs; every word of ``scale_permuted`` is
    written.  ``hidden_states_scale`` goes in by its strides: it is not copied."""
    T, top_k = topk_ids.shape
    n, G, dev = T * top_k, local_num_experts, hidden_states.device
    blocks = -(-n // _lib.FI_MOE_SORT_BLOCK)
    workspace = torch.empty((blocks * G + n,), dtype=torch.int32, device=dev)
    ids, x = topk_ids.contiguous(), contiguous_aligned(hidden_states, 16)
    p = _lib.fi_moe_permute_fp8_block_params_t(
        topk_ids=ids.data_ptr(), x=x.data_ptr(), x_scale=hidden_states_scale.data_ptr(), m_indptr=m_indptr.data_ptr(),
        expanded_to_permuted=emap.data_ptr(), x_permuted=x_permuted.data_ptr(), scale_permuted=scale_permuted.data_ptr(),
        unpacked_weights=_lib.ptr(weights), workspace=workspace.data_ptr(),
        scale_stride_kb=hidden_states_scale.stride(0), scale_stride_t=hidden_states_scale.stride(1),
        workspace_bytes=_lib.nbytes(workspace), num_tokens=T, top_k=top_k, hidden=hidden_states.shape[1],
        local_expert_offset=local_expert_offset, local_num_experts=G, packed=int(bool(packed)))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().fi_moe_permute_fp8_block(C.byref(p), _lib.current_stream(dev)), "moe_permute_fp8_block")


def moe_permute_fp8_block(
    topk_ids: torch.Tensor,
    hidden_states: torch.Tensor,
    hidden_states_scale: torch.Tensor,
    local_expert_offset: int,
    local_num_experts: int,
    packed: bool = False,
) -> Tuple[torch.Tensor, ...]:
    """``moe_permute_mxfp8`` for fp8 block-scale activations: the row operand of GEMM1 of ``trtllm_fp8_block_scale_moe``.
    Not part of the reference.

    ``topk_ids`` as there.  ``hidden_states`` float8_e4m3fn ``[T, H]`` and ``hidden_states_scale`` float32 ``[H / 128, T]``
    with any strides (contiguous, or the ``.t()`` view of a ``[T, H / 128]`` tensor): it is read through them, not copied.
    Returns ``(m_indptr, expanded_idx_to_permuted_idx, x_permuted, scale_permuted)`` and with ``packed`` the bf16 weights:

    * ``m_indptr`` and ``expanded_idx_to_permuted_idx``: what ``moe_permute_mxfp8`` returns for the same ids;
    * ``x_permuted`` float8_e4m3fn ``[T * top_k, H]``; rows at or past ``m_indptr[-1]`` are unwritten;
    * ``scale_permuted`` float32 ``[T * top_k, H / 128]`` row-major, the ``a_scale`` of ``group_gemm_fp8_nt_groupwise`` in
      its ``"K"`` mode; rows at or past ``m_indptr[-1]`` are 1.0.
    """
    if topk_ids.dtype != torch.int32 or topk_ids.dim() != 2:
        raise ValueError("topk_ids must be a 2D int32 tensor (T, top_k)")
    _check_fp8_block_activations(hidden_states, hidden_states_scale)
    T, top_k = topk_ids.shape
    H = hidden_states.shape[1]
    if hidden_states.shape[0] != T:
        raise ValueError(f"topk_ids has {T} rows, hidden_states {hidden_states.shape[0]}")
    if not 1 <= top_k <= _MAX_TOP_K:
        raise NotImplementedError(f"top_k {top_k} is not in [1, {_MAX_TOP_K}]")
    if not 1 <= local_num_experts <= _MAX_EXPERTS or local_expert_offset < 0:
        raise NotImplementedError(
            f"local_num_experts {local_num_experts} is not in [1, {_MAX_EXPERTS}] or local_expert_offset {local_expert_offset} < 0")
    for t, name in ((topk_ids, "topk_ids"), (hidden_states, "hidden_states"), (hidden_states_scale, "hidden_states_scale")):
        _lib.require_gpu_tensor(t, name)
    dev = hidden_states.device
    n, G = T * top_k, local_num_experts
    m_indptr = torch.empty((G + 1,), dtype=torch.int32, device=dev)
    emap = torch.empty((n,), dtype=torch.int32, device=dev)
    x_permuted = torch.empty((n, H), dtype=torch.float8_e4m3fn, device=dev)
    scale_permuted = torch.empty((n, H // _FP8_BLOCK), dtype=torch.float32, device=dev)
    weights = torch.empty((T, top_k), dtype=torch.bfloat16, device=dev) if packed else None
    if T == 0:
        m_indptr.zero_()
    else:
        _permute_fp8_block_into(topk_ids, hidden_states, hidden_states_scale, local_expert_offset, G, packed, m_indptr,
                                emap, x_permuted, scale_permuted, weights)
    if packed:
        return m_indptr, emap, x_permuted, scale_permuted, weights
    return m_indptr, emap, x_permuted, scale_permuted


def _gated_act_fp8_block_into(gemm1_output: torch.Tensor, m_indptr: torch.Tensor, q: torch.Tensor,
                              scale: torch.Tensor) -> None:
    """fi_moe_gated_act_fp8_block on checked tensors (cum_m > 0) into pre-allocated outputs; every word of ``scale`` is
    written, rows of ``q`` at or past ``m_indptr[-1]`` are not."""
    cum_m, two_i = gemm1_output.shape
    dev = gemm1_output.device
    x = contiguous_aligned(gemm1_output, 16)
    p = _lib.fi_moe_gated_act_fp8_block_params_t(
        x=x.data_ptr(), m_indptr=m_indptr.contiguous().data_ptr(), q=q.data_ptr(), scale=scale.data_ptr(), cum_m=cum_m,
        intermediate=two_i // 2, num_groups=m_indptr.shape[0] - 1)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().fi_moe_gated_act_fp8_block(C.byref(p), _lib.current_stream(dev)), "moe_gated_act_fp8_block")


def moe_gated_act_fp8_block(gemm1_output: torch.Tensor, m_indptr: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """SwiGLU between the two GEMMs of ``trtllm_fp8_block_scale_moe``, quantised to fp8 with one f32 scale per row and 128
    columns for the second.  Not part of the reference.

    ``gemm1_output`` is bf16 ``[cum_m, 2 I]`` with ``I % 128 == 0``: columns ``[0, I)`` the linear half ``x1``, ``[I, 2 I)`` the
    gate ``x2``.  In f32 ``act = x2 * sigmoid(x2) * x1``; the fp8 call has no bias, alpha, beta or limit.  Per row and block
    of 128 columns ``s = max(amax / 448, 2^-126)`` and ``q = e4m3(clamp(act / s, -448, 448))``, the rule and the device code
    of ``fp8_quantize_1x128``.  Returns ``(q, scale)``: float8_e4m3fn ``[cum_m, I]`` and float32 ``[cum_m, I / 128]`` row-major.
    Rows at or past ``m_indptr[-1]``: ``q`` is not written, ``scale`` is 1.0.
    """
    if gemm1_output.dtype != torch.bfloat16 or gemm1_output.dim() != 2:
        raise ValueError("gemm1_output must be a 2D bfloat16 tensor (cum_m, 2 I)")
    if m_indptr.dtype != torch.int32 or m_indptr.dim() != 1 or m_indptr.shape[0] < 2:
        raise ValueError("m_indptr must be a 1D int32 tensor of G + 1 >= 2 entries")
    cum_m, two_i = gemm1_output.shape
    I, G = two_i // 2, m_indptr.shape[0] - 1
    if two_i == 0 or two_i % 256 != 0:
        raise NotImplementedError(f"intermediate_size {two_i / 2:g} must be a multiple of 128")
    if G > _MAX_EXPERTS:
        raise NotImplementedError(f"{G} groups: at most {_MAX_EXPERTS}")
    _lib.require_gpu_tensor(gemm1_output, "gemm1_output")
    _lib.require_gpu_tensor(m_indptr, "m_indptr")
    dev = gemm1_output.device
    q = torch.empty((cum_m, I), dtype=torch.float8_e4m3fn, device=dev)
    scale = torch.empty((cum_m, I // _FP8_BLOCK), dtype=torch.float32, device=dev)
    if cum_m:
        _gated_act_fp8_block_into(gemm1_output, m_indptr, q, scale)
    return q, scale
