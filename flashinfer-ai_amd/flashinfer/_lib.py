"""ctypes binding of libfi_mi355.so (the C ABI declared in include/fi_mi355.h).

The reference loads one JIT-built module per kernel specialisation through tvm_ffi
(ref: flashinfer/jit/core.py:247-263); here ONE ahead-of-time library serves every op.  There is no
fallback: if the library is missing every op raises (a CPU path would void the parity claims).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("FI_MI355_LIB", os.path.join(_HERE, "libfi_mi355.so"))

FI_DTYPE_F16, FI_DTYPE_BF16, FI_DTYPE_FP8_E4M3, FI_DTYPE_FP8_E5M2, FI_DTYPE_F32 = range(5)
FI_NEG_INF = -5.0e4
FI_DECODE_PLAN_INFO_LEN = 17
FI_DP_UNIFORM_CHUNKS = 16  # plan_info slot: 2 | 4 when every request is cut into that many chunks, else 0

_TORCH2FI = {
    torch.float16: FI_DTYPE_F16,
    torch.bfloat16: FI_DTYPE_BF16,
    torch.float8_e4m3fn: FI_DTYPE_FP8_E4M3,
    torch.float8_e5m2: FI_DTYPE_FP8_E5M2,
    torch.float32: FI_DTYPE_F32,
}


def fi_dtype(dtype: torch.dtype) -> int:
    try:
        return _TORCH2FI[dtype]
    except KeyError:
        raise ValueError(f"unsupported dtype {dtype} for the MI355X kernels") from None


class PagedKV(C.Structure):
    _fields_ = [
        ("k_data", C.c_void_p),
        ("v_data", C.c_void_p),
        ("indptr", C.c_void_p),
        ("indices", C.c_void_p),
        ("last_page_len", C.c_void_p),
        ("rope_pos_offset", C.c_void_p),
        ("stride_page", C.c_int64),
        ("stride_n", C.c_int64),
        ("stride_h", C.c_int64),
        ("page_size", C.c_int32),
        ("num_kv_heads", C.c_int32),
        ("head_dim", C.c_int32),
        ("batch_size", C.c_int32),
        ("dtype", C.c_int32),
    ]


class BatchDecodeParams(C.Structure):
    _fields_ = [
        ("q", C.c_void_p),
        ("q_stride_n", C.c_int64),
        ("q_stride_h", C.c_int64),
        ("kv", PagedKV),
        ("o", C.c_void_p),
        ("lse", C.c_void_p),
        ("alibi_slopes", C.c_void_p),
        ("q_rope_offset", C.c_void_p),
        ("num_qo_heads", C.c_int32),
        ("q_dtype", C.c_int32),
        ("pos_encoding_mode", C.c_int32),
        ("window_left", C.c_int32),
        ("logits_soft_cap", C.c_float),
        ("sm_scale", C.c_float),
        ("rope_rcp_scale", C.c_float),
        ("rope_rcp_theta", C.c_float),
    ]


class SingleDecodeParams(C.Structure):
    _fields_ = [
        ("q", C.c_void_p),
        ("q_stride_h", C.c_int64),
        ("k", C.c_void_p),
        ("v", C.c_void_p),
        ("kv_stride_n", C.c_int64),
        ("kv_stride_h", C.c_int64),
        ("o", C.c_void_p),
        ("lse", C.c_void_p),
        ("alibi_slopes", C.c_void_p),
        ("kv_len", C.c_int32),
        ("num_qo_heads", C.c_int32),
        ("num_kv_heads", C.c_int32),
        ("head_dim", C.c_int32),
        ("q_dtype", C.c_int32),
        ("kv_dtype", C.c_int32),
        ("pos_encoding_mode", C.c_int32),
        ("window_left", C.c_int32),
        ("logits_soft_cap", C.c_float),
        ("sm_scale", C.c_float),
        ("rope_rcp_scale", C.c_float),
        ("rope_rcp_theta", C.c_float),
    ]


class BatchPrefillParams(C.Structure):
    _fields_ = [
        ("q", C.c_void_p),
        ("q_stride_n", C.c_int64),
        ("q_stride_h", C.c_int64),
        ("qo_indptr", C.c_void_p),
        ("kv", PagedKV),
        ("o", C.c_void_p),
        ("lse", C.c_void_p),
        ("alibi_slopes", C.c_void_p),
        ("scale_q", C.c_void_p),
        ("scale_k", C.c_void_p),
        ("scale_v", C.c_void_p),
        ("custom_mask", C.c_void_p),
        ("mask_indptr", C.c_void_p),
        ("prefix_len_ptr", C.c_void_p),
        ("token_pos_in_items_ptr", C.c_void_p),
        ("max_item_len_ptr", C.c_void_p),
        ("token_pos_in_items_len", C.c_int32),
        ("num_qo_heads", C.c_int32),
        ("q_dtype", C.c_int32),
        ("o_dtype", C.c_int32),
        ("mask_mode", C.c_int32),
        ("pos_encoding_mode", C.c_int32),
        ("window_left", C.c_int32),
        ("logits_soft_cap", C.c_float),
        ("sm_scale", C.c_float),
        ("rope_rcp_scale", C.c_float),
        ("rope_rcp_theta", C.c_float),
        ("bf16_pv_mode", C.c_int32),
    ]


class SinglePrefillParams(C.Structure):
    _fields_ = [
        ("q", C.c_void_p),
        ("q_stride_n", C.c_int64),
        ("q_stride_h", C.c_int64),
        ("k", C.c_void_p),
        ("v", C.c_void_p),
        ("kv_stride_n", C.c_int64),
        ("kv_stride_h", C.c_int64),
        ("o", C.c_void_p),
        ("lse", C.c_void_p),
        ("alibi_slopes", C.c_void_p),
        ("scale_q", C.c_void_p),
        ("scale_k", C.c_void_p),
        ("scale_v", C.c_void_p),
        ("custom_mask", C.c_void_p),
        ("qo_len", C.c_int32),
        ("kv_len", C.c_int32),
        ("num_qo_heads", C.c_int32),
        ("num_kv_heads", C.c_int32),
        ("head_dim", C.c_int32),
        ("q_dtype", C.c_int32),
        ("kv_dtype", C.c_int32),
        ("o_dtype", C.c_int32),
        ("mask_mode", C.c_int32),
        ("pos_encoding_mode", C.c_int32),
        ("window_left", C.c_int32),
        ("logits_soft_cap", C.c_float),
        ("sm_scale", C.c_float),
        ("rope_rcp_scale", C.c_float),
        ("rope_rcp_theta", C.c_float),
        ("bf16_pv_mode", C.c_int32),
    ]


class PrefillQkvoParams(C.Structure):
    """fi_prefill_qkvo_params_t: prefill with head_dim_qk 192 / head_dim_vo 128 (batch ragged or single)."""
    _fields_ = [
        ("q", C.c_void_p),
        ("q_stride_n", C.c_int64),
        ("q_stride_h", C.c_int64),
        ("k", C.c_void_p),
        ("k_stride_n", C.c_int64),
        ("k_stride_h", C.c_int64),
        ("v", C.c_void_p),
        ("v_stride_n", C.c_int64),
        ("v_stride_h", C.c_int64),
        ("o", C.c_void_p),
        ("lse", C.c_void_p),
        ("qo_indptr", C.c_void_p),
        ("kv_indptr", C.c_void_p),
        ("batch_size", C.c_int32),
        ("qo_len", C.c_int32),
        ("kv_len", C.c_int32),
        ("num_qo_heads", C.c_int32),
        ("num_kv_heads", C.c_int32),
        ("head_dim_qk", C.c_int32),
        ("head_dim_vo", C.c_int32),
        ("q_dtype", C.c_int32),
        ("kv_dtype", C.c_int32),
        ("o_dtype", C.c_int32),
        ("mask_mode", C.c_int32),
        ("pos_encoding_mode", C.c_int32),
        ("window_left", C.c_int32),
        ("logits_soft_cap", C.c_float),
        ("sm_scale", C.c_float),
        ("bf16_pv_mode", C.c_int32),
    ]


class RopeParams(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("q_out", C.c_void_p), ("k_out", C.c_void_p),
        ("pos_ids", C.c_void_p), ("cos_sin_cache", C.c_void_p),
        ("q_stride_n", C.c_int64), ("q_stride_h", C.c_int64), ("k_stride_n", C.c_int64), ("k_stride_h", C.c_int64),
        ("qo_stride_n", C.c_int64), ("qo_stride_h", C.c_int64), ("ko_stride_n", C.c_int64), ("ko_stride_h", C.c_int64),
        ("nnz", C.c_int32), ("num_q_heads", C.c_int32), ("num_k_heads", C.c_int32), ("head_dim", C.c_int32),
        ("rotary_dim", C.c_int32), ("interleave", C.c_int32), ("dtype", C.c_int32),
        ("rope_rcp_scale", C.c_float), ("rope_rcp_theta", C.c_float), ("smooth_a", C.c_float), ("smooth_b", C.c_float),
    ]


class MlaPlanParams(C.Structure):
    _fields_ = [
        ("int_ws", C.c_void_p), ("pinned_int_ws", C.c_void_p), ("int_ws_bytes", C.c_size_t),
        ("float_ws_bytes", C.c_size_t), ("qo_indptr_h", C.c_void_p), ("kv_indptr_h", C.c_void_p),
        ("kv_len_arr_h", C.c_void_p), ("batch_size", C.c_int32), ("num_heads", C.c_int32),
        ("head_dim_ckv", C.c_int32), ("head_dim_kpe", C.c_int32), ("page_size", C.c_int32), ("causal", C.c_int32),
        ("q_dtype", C.c_int32), ("kv_dtype", C.c_int32), ("enable_cuda_graph", C.c_int32),
        ("fixed_split_size", C.c_int32),
    ]


class MlaParams(C.Structure):
    _fields_ = [
        ("q_nope", C.c_void_p), ("q_nope_stride_n", C.c_int64), ("q_nope_stride_h", C.c_int64),
        ("q_pe", C.c_void_p), ("q_pe_stride_n", C.c_int64), ("q_pe_stride_h", C.c_int64),
        ("ckv", C.c_void_p), ("ckv_stride_page", C.c_int64), ("ckv_stride_n", C.c_int64),
        ("kpe", C.c_void_p), ("kpe_stride_page", C.c_int64), ("kpe_stride_n", C.c_int64),
        ("kv_indices", C.c_void_p), ("o", C.c_void_p), ("lse", C.c_void_p),
        ("float_ws", C.c_void_p), ("float_ws_bytes", C.c_size_t), ("int_ws", C.c_void_p), ("int_ws_bytes", C.c_size_t),
        ("num_rows", C.c_int32), ("num_heads", C.c_int32), ("page_size", C.c_int32), ("dtype", C.c_int32),
        ("causal", C.c_int32), ("sm_scale", C.c_float),
    ]


class AppendMlaParams(C.Structure):
    _fields_ = [
        ("append_ckv", C.c_void_p), ("append_ckv_stride_n", C.c_int64),
        ("append_kpe", C.c_void_p), ("append_kpe_stride_n", C.c_int64),
        ("batch_indices", C.c_void_p), ("positions", C.c_void_p),
        ("ckv_cache", C.c_void_p), ("ckv_stride_page", C.c_int64), ("ckv_stride_n", C.c_int64),
        ("kpe_cache", C.c_void_p), ("kpe_stride_page", C.c_int64), ("kpe_stride_n", C.c_int64),
        ("kv_indices", C.c_void_p), ("kv_indptr", C.c_void_p),
        ("nnz", C.c_int32), ("page_size", C.c_int32), ("head_dim_ckv", C.c_int32), ("head_dim_kpe", C.c_int32),
        ("dtype", C.c_int32),
    ]


class SamplingParams(C.Structure):
    """fi_sampling_params_t: the draws (plain, from logits, top-k / top-p / min-p / joint)."""
    _fields_ = [
        ("probs", C.c_void_p), ("samples", C.c_void_p), ("indices", C.c_void_p),
        ("top_k_arr", C.c_void_p), ("top_p_arr", C.c_void_p),
        ("top_k_val", C.c_int32), ("top_p_val", C.c_float),
        ("batch", C.c_int32), ("num_rows", C.c_int32), ("vocab", C.c_int32), ("param_len", C.c_int32),
        ("philox_seed", C.c_uint64), ("philox_offset", C.c_uint64),
    ]


class RowTransformParams(C.Structure):
    """fi_row_transform_params_t: softmax, top-p / top-k renormalisation, top-k logit mask."""
    _fields_ = [
        ("in_", C.c_void_p), ("out", C.c_void_p), ("top_k_arr", C.c_void_p), ("scalar_arr", C.c_void_p),
        ("top_k_val", C.c_int32), ("scalar_val", C.c_float),
        ("batch", C.c_int32), ("vocab", C.c_int32), ("param_len", C.c_int32),
    ]


class ChainSpeculativeParams(C.Structure):
    _fields_ = [
        ("draft_probs", C.c_void_p), ("draft_token_ids", C.c_void_p), ("target_probs", C.c_void_p),
        ("output_token_ids", C.c_void_p), ("output_accepted_token_num", C.c_void_p),
        ("output_emitted_draft_token_num", C.c_void_p),
        ("batch", C.c_int32), ("num_speculative_tokens", C.c_int32), ("vocab", C.c_int32),
        ("philox_seed", C.c_uint64), ("philox_offset", C.c_uint64),
    ]


class RmsNormParams(C.Structure):
    """fi_rmsnorm_params_t: RMSNorm over [batch, hidden] (num_heads == 1) or [batch, num_heads, hidden]."""
    _fields_ = [
        ("in_", C.c_void_p), ("weight", C.c_void_p), ("out", C.c_void_p),
        ("batch", C.c_int32), ("num_heads", C.c_int32), ("hidden", C.c_int32),
        ("in_stride_n", C.c_int64), ("in_stride_h", C.c_int64), ("out_stride_n", C.c_int64), ("out_stride_h", C.c_int64),
        ("eps", C.c_float), ("weight_bias", C.c_float), ("dtype", C.c_int32),
    ]


class FusedAddRmsNormParams(C.Structure):
    _fields_ = [
        ("input", C.c_void_p), ("residual", C.c_void_p), ("weight", C.c_void_p),
        ("batch", C.c_int32), ("hidden", C.c_int32), ("input_stride", C.c_int64), ("residual_stride", C.c_int64),
        ("eps", C.c_float), ("weight_bias", C.c_float), ("dtype", C.c_int32),
    ]


class ActAndMulParams(C.Structure):
    _fields_ = [
        ("in_", C.c_void_p), ("out", C.c_void_p), ("tokens", C.c_int64), ("d", C.c_int32), ("act", C.c_int32),
        ("dtype", C.c_int32),
    ]


FI_NORM_MAX_HIDDEN = 65536
FI_ACT_SILU, FI_ACT_GELU, FI_ACT_GELU_TANH = range(3)

FI_PREFILL_PLAN_INFO_LEN = 16
FI_PREFILL_PLAN_MAGIC = 0x4649505245
FI_PREFILL_QKVO_PLAN_MAGIC = 0x4649514B564F  # plan_info[15] of a head_dim_qk 192 / head_dim_vo 128 plan
FI_MLA_PLAN_INFO_LEN = 16
# plan_info slots of fi_batch_mla_plan (include/fi_mi355.h, enum fi_mla_plan_slot)
(FI_MLA_NUM_WORK, FI_MLA_GRID, FI_MLA_TOTAL_ROWS, FI_MLA_KV_CHUNK_SIZE, FI_MLA_SPLIT_KV, FI_MLA_ENABLE_CUDA_GRAPH,
 FI_MLA_NUM_HEADS, FI_MLA_BATCH_SIZE, FI_MLA_INT_BYTES_USED, FI_MLA_MERGE_INDPTR_OFFSET, FI_MLA_ITEMS_OFFSET,
 FI_MLA_NUM_ENTRIES, FI_MLA_V_OFFSET, FI_MLA_PAGE_SIZE, FI_MLA_DTYPE, FI_MLA_MAGIC) = range(16)

_lib: Optional[C.CDLL] = None

# every symbol include/fi_mi355.h declares; tests check the library exports all of them
EXPORTED_SYMBOLS = [
    "fi_last_error",
    "fi_abi_version",
    "fi_num_compute_units",
    "fi_batch_decode_plan",
    "fi_batch_decode_run",
    "fi_batch_decode_run_sinks",
    "fi_single_decode_run",
    "fi_merge_state",
    "fi_merge_state_in_place",
    "fi_merge_states",
    "fi_variable_length_merge_states",
    "fi_batch_prefill_plan",
    "fi_batch_prefill_paged_run",
    "fi_batch_prefill_paged_run_sinks",
    "fi_single_prefill_run",
    "fi_batch_prefill_qkvo_run",
    "fi_single_prefill_qkvo_run",
    "fi_gemm_fp8_nt_groupwise",
    "fi_group_gemm_fp8_nt_groupwise",
    "fi_get_batch_indices_positions",
    "fi_append_paged_kv_cache",
    "fi_apply_rope_pos_ids",
    "fi_apply_rope_append_paged_kv_cache",
    "fi_rope_positions_from_indptr",
    "fi_packbits",
    "fi_segment_packbits",
    "fi_batch_mla_plan",
    "fi_batch_mla_run",
    "fi_append_paged_mla_kv_cache",
    "fi_softmax",
    "fi_sampling_from_logits",
    "fi_sampling_from_probs",
    "fi_top_k_sampling_from_probs",
    "fi_top_p_sampling_from_probs",
    "fi_min_p_sampling_from_probs",
    "fi_top_k_top_p_sampling_from_probs",
    "fi_top_p_renorm_probs",
    "fi_top_k_renorm_probs",
    "fi_top_k_mask_logits",
    "fi_chain_speculative_sampling",
    "fi_rmsnorm",
    "fi_fused_add_rmsnorm",
    "fi_act_and_mul",
]

SAMPLING_SYMBOLS = ("fi_sampling_from_logits", "fi_sampling_from_probs", "fi_top_k_sampling_from_probs",
                    "fi_top_p_sampling_from_probs", "fi_min_p_sampling_from_probs",
                    "fi_top_k_top_p_sampling_from_probs")
ROW_TRANSFORM_SYMBOLS = ("fi_softmax", "fi_top_p_renorm_probs", "fi_top_k_renorm_probs", "fi_top_k_mask_logits")


def lib() -> C.CDLL:
    """Load the library (once).  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"{_LIB_PATH} not found: build it with `make -C flashinfer-ai_amd/csrc -j8` "
            "(or python -c 'import __graft_entry__ as g; g.build()').  There is no CPU fallback."
        )
    l = C.CDLL(_LIB_PATH)
    l.fi_last_error.restype = C.c_char_p
    l.fi_abi_version.restype = C.c_int
    l.fi_num_compute_units.restype = C.c_int
    vp, i32, i64p, sz = C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_size_t
    l.fi_batch_decode_plan.argtypes = [vp, sz, vp, vp, sz, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i64p, vp]
    l.fi_batch_decode_run.argtypes = [vp, sz, vp, sz, i64p, i32, C.POINTER(BatchDecodeParams), vp]
    l.fi_batch_decode_run_sinks.argtypes = [vp, sz, vp, sz, i64p, i32, C.POINTER(BatchDecodeParams), vp, vp]
    l.fi_single_decode_run.argtypes = [C.POINTER(SingleDecodeParams), vp, sz, vp]
    l.fi_merge_state.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    l.fi_merge_state_in_place.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    l.fi_merge_states.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    l.fi_variable_length_merge_states.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    l.fi_batch_prefill_plan.argtypes = [vp, sz, vp, vp, sz, vp, vp, vp] + [i32] * 12 + [i64p, vp]
    l.fi_batch_prefill_paged_run.argtypes = [vp, sz, vp, sz, i64p, i32, C.POINTER(BatchPrefillParams), vp]
    l.fi_batch_prefill_paged_run_sinks.argtypes = [vp, sz, vp, sz, i64p, i32, C.POINTER(BatchPrefillParams), vp, vp]
    l.fi_single_prefill_run.argtypes = [C.POINTER(SinglePrefillParams), vp, sz, vp]
    l.fi_batch_prefill_qkvo_run.argtypes = [vp, sz, vp, sz, i64p, i32, C.POINTER(PrefillQkvoParams), vp]
    l.fi_single_prefill_qkvo_run.argtypes = [C.POINTER(PrefillQkvoParams), vp, sz, vp]
    l.fi_gemm_fp8_nt_groupwise.argtypes = [vp] * 5 + [i32] * 10 + [vp]
    l.fi_group_gemm_fp8_nt_groupwise.argtypes = [vp] * 6 + [i32] * 11 + [vp]
    l.fi_packbits.argtypes = [vp, C.c_int64, i32, vp, vp]
    l.fi_segment_packbits.argtypes = [vp, vp, vp, i32, C.c_int64, i32, vp, vp]
    l.fi_get_batch_indices_positions.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    l.fi_append_paged_kv_cache.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, vp, vp, i32, C.POINTER(PagedKV), vp]
    l.fi_apply_rope_pos_ids.argtypes = [C.POINTER(RopeParams), vp]
    l.fi_apply_rope_append_paged_kv_cache.argtypes = [C.POINTER(RopeParams), vp, C.c_int64, C.c_int64, vp, vp, C.POINTER(PagedKV), vp]
    l.fi_rope_positions_from_indptr.argtypes = [vp, vp, i32, i32, vp, vp]
    l.fi_batch_mla_plan.argtypes = [C.POINTER(MlaPlanParams), i64p, vp]
    l.fi_batch_mla_run.argtypes = [i64p, i32, C.POINTER(MlaParams), vp]
    l.fi_append_paged_mla_kv_cache.argtypes = [C.POINTER(AppendMlaParams), vp]
    for name in SAMPLING_SYMBOLS:
        getattr(l, name).argtypes = [C.POINTER(SamplingParams), vp]
    for name in ROW_TRANSFORM_SYMBOLS:
        getattr(l, name).argtypes = [C.POINTER(RowTransformParams), vp]
    l.fi_chain_speculative_sampling.argtypes = [C.POINTER(ChainSpeculativeParams), vp]
    l.fi_rmsnorm.argtypes = [C.POINTER(RmsNormParams), vp]
    l.fi_fused_add_rmsnorm.argtypes = [C.POINTER(FusedAddRmsNormParams), vp]
    l.fi_act_and_mul.argtypes = [C.POINTER(ActAndMulParams), vp]
    for name in EXPORTED_SYMBOLS:
        fn = getattr(l, name)
        if name not in ("fi_last_error",):
            fn.restype = C.c_int
    _lib = l
    return l


def check(status: int, what: str) -> None:
    """Turn a non-zero status into a Python exception carrying fi_last_error().
    (ref: TVM_FFI_ICHECK / FLASHINFER_ERROR surface as Python exceptions.)"""
    if status != 0:
        msg = lib().fi_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed: {msg}")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def nbytes(t: torch.Tensor) -> int:
    """Size of a tensor's elements in bytes: what the C ABI takes wherever it takes a buffer size."""
    return t.numel() * t.element_size()


def current_stream(device: torch.device) -> int:
    """hipStream_t of torch's current stream on `device` (ref: csrc/tvm_ffi_utils.h:256-264)."""
    return torch.cuda.current_stream(device).cuda_stream


def batch_decode_plan(float_ws, int_ws, pinned_int_ws, indptr_host, batch_size, num_qo_heads, num_kv_heads, page_size,
                      enable_cuda_graph, head_dim, q_dtype, kv_dtype, max_grid_hint, window_left, what: str):
    """fi_batch_decode_plan on the float workspace's device; returns the plan_info array.  ``indptr_host`` is the
    host copy of the page-table prefix sums, ``q_dtype`` / ``kv_dtype`` are torch dtypes."""
    info = (C.c_int64 * FI_DECODE_PLAN_INFO_LEN)()
    with torch.cuda.device(float_ws.device):
        check(
            lib().fi_batch_decode_plan(
                float_ws.data_ptr(), nbytes(float_ws), int_ws.data_ptr(), pinned_int_ws.data_ptr(), nbytes(int_ws),
                indptr_host.data_ptr(), batch_size, num_qo_heads, num_kv_heads, page_size, int(enable_cuda_graph),
                head_dim, fi_dtype(q_dtype), fi_dtype(kv_dtype), max_grid_hint, window_left, info,
                current_stream(float_ws.device),
            ),
            what,
        )
    return info


def batch_prefill_plan(float_ws, int_ws, pinned_int_ws, qo_indptr_host, kv_indptr_host, kv_len_arr_host,
                       total_num_rows, batch_size, num_qo_heads, num_kv_heads, page_size, enable_cuda_graph,
                       head_dim_qk, head_dim_vo, causal, window_left, fixed_split_size, disable_split_kv, what: str):
    """fi_batch_prefill_plan on the float workspace's device; returns the plan_info array.  The three index tensors
    are host int32 tensors; ``fixed_split_size`` is -1 for the planner's own choice."""
    info = (C.c_int64 * FI_PREFILL_PLAN_INFO_LEN)()
    with torch.cuda.device(float_ws.device):
        check(
            lib().fi_batch_prefill_plan(
                float_ws.data_ptr(), nbytes(float_ws), int_ws.data_ptr(), pinned_int_ws.data_ptr(), nbytes(int_ws),
                qo_indptr_host.data_ptr(), kv_indptr_host.data_ptr(), kv_len_arr_host.data_ptr(), total_num_rows,
                batch_size, num_qo_heads, num_kv_heads, page_size, int(enable_cuda_graph), head_dim_qk, head_dim_vo,
                int(causal), window_left, fixed_split_size, int(disable_split_kv), info,
                current_stream(float_ws.device),
            ),
            what,
        )
    return info


def require_gpu_tensor(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} must live on a GPU (got {t.device}); the MI355X kernels have no CPU fallback"
        )
