"""flashinfer -- MI355X (gfx950) native implementation of FlashInfer's paged-KV attention hot path.

Drop-in for the ``flashinfer.decode / prefill / attention (sinks) / cascade / page / sparse / gemm / fused_moe / fused_moe_fp8 / fp8_quantization / fp4_quantization / sampling / norm / activation / rope / mla`` operator API
of FlashInfer v0.3.1 (ref: flashinfer/__init__.py:23-145), backed by hand-written HIP kernels behind the C ABI of
``libfi_mi355.so`` (include/fi_mi355.h).  Only the path named in DESIGN.md is provided; of the fp4 matmuls that is
``mm_fp4`` in its MXFP4 mode (``use_nvfp4=False, block_size=32``), not nvfp4.
"""
from . import _lib as _lib
from . import activation as activation
from . import fp4_quantization as fp4_quantization
from . import fp8_quantization as fp8_quantization
from . import fused_moe as fused_moe
from . import fused_moe_fp8 as fused_moe_fp8
from . import mla as mla
from . import norm as norm
from . import sampling as sampling
from . import sparse as sparse
from .activation import gelu_and_mul as gelu_and_mul
from .activation import gelu_tanh_and_mul as gelu_tanh_and_mul
from .activation import silu_and_mul as silu_and_mul
from .attention import (
    BatchAttentionWithAttentionSinkWrapper as BatchAttentionWithAttentionSinkWrapper,
)
from .cascade import (
    BatchDecodeWithSharedPrefixPagedKVCacheWrapper as BatchDecodeWithSharedPrefixPagedKVCacheWrapper,
)
from .cascade import (
    BatchPrefillWithSharedPrefixPagedKVCacheWrapper as BatchPrefillWithSharedPrefixPagedKVCacheWrapper,
)
from .cascade import (
    MultiLevelCascadeAttentionWrapper as MultiLevelCascadeAttentionWrapper,
)
from .cascade import merge_state as merge_state
from .cascade import merge_state_in_place as merge_state_in_place
from .cascade import merge_states as merge_states
from .decode import (
    BatchDecodeWithPagedKVCacheWrapper as BatchDecodeWithPagedKVCacheWrapper,
)
from .decode import (
    CUDAGraphBatchDecodeWithPagedKVCacheWrapper as CUDAGraphBatchDecodeWithPagedKVCacheWrapper,
)
from .decode import fast_decode_plan as fast_decode_plan
from .decode import single_decode_with_kv_cache as single_decode_with_kv_cache
from .fp4_quantization import block_scale_interleave as block_scale_interleave
from .fp4_quantization import e2m1_and_ufp8sf_scale_to_float as e2m1_and_ufp8sf_scale_to_float
from .fp4_quantization import fp4_quantize as fp4_quantize
from .fp4_quantization import mxfp4_dequantize as mxfp4_dequantize
from .fp4_quantization import mxfp4_dequantize_host as mxfp4_dequantize_host
from .fp4_quantization import mxfp4_quantize as mxfp4_quantize
from .fp4_quantization import mxfp4_quantize_grouped as mxfp4_quantize_grouped
from .fp4_quantization import nvfp4_block_scale_interleave as nvfp4_block_scale_interleave
from .fp8_quantization import mxfp8_dequantize_host as mxfp8_dequantize_host
from .fp8_quantization import mxfp8_quantize as mxfp8_quantize
from .fused_moe import GatedActType as GatedActType
from .fused_moe import RoutingMethodType as RoutingMethodType
from .fused_moe import trtllm_fp4_block_scale_moe as trtllm_fp4_block_scale_moe
from .fused_moe import (
    trtllm_fp4_block_scale_routed_moe as trtllm_fp4_block_scale_routed_moe,
)
from .gemm import gemm_fp8_nt_groupwise as gemm_fp8_nt_groupwise
from .gemm import group_gemm_fp8_nt_groupwise as group_gemm_fp8_nt_groupwise
from .gemm import mm_fp4 as mm_fp4
from .mla import BatchMLAPagedAttentionWrapper as BatchMLAPagedAttentionWrapper
from .norm import fused_add_rmsnorm as fused_add_rmsnorm
from .norm import gemma_fused_add_rmsnorm as gemma_fused_add_rmsnorm
from .norm import gemma_rmsnorm as gemma_rmsnorm
from .norm import rmsnorm as rmsnorm
from .page import append_paged_kv_cache as append_paged_kv_cache
from .page import append_paged_mla_kv_cache as append_paged_mla_kv_cache
from .page import apply_rope_append_paged_kv_cache as apply_rope_append_paged_kv_cache
from .page import (
    block_sparse_indices_to_vector_sparse_offsets as block_sparse_indices_to_vector_sparse_offsets,
)
from .page import get_batch_indices_positions as get_batch_indices_positions
from .page import get_seq_lens as get_seq_lens
from .prefill import (
    BatchPrefillWithPagedKVCacheWrapper as BatchPrefillWithPagedKVCacheWrapper,
)
from .prefill import (
    BatchPrefillWithRaggedKVCacheWrapper as BatchPrefillWithRaggedKVCacheWrapper,
)
from .prefill import single_prefill_with_kv_cache as single_prefill_with_kv_cache
from .prefill import (
    single_prefill_with_kv_cache_return_lse as single_prefill_with_kv_cache_return_lse,
)
from .quantization import packbits as packbits
from .quantization import segment_packbits as segment_packbits
from .rope import apply_llama31_rope as apply_llama31_rope
from .rope import apply_llama31_rope_inplace as apply_llama31_rope_inplace
from .rope import apply_llama31_rope_pos_ids as apply_llama31_rope_pos_ids
from .rope import (
    apply_llama31_rope_pos_ids_inplace as apply_llama31_rope_pos_ids_inplace,
)
from .rope import apply_rope as apply_rope
from .rope import apply_rope_inplace as apply_rope_inplace
from .rope import apply_rope_pos_ids as apply_rope_pos_ids
from .rope import apply_rope_pos_ids_inplace as apply_rope_pos_ids_inplace
from .rope import apply_rope_with_cos_sin_cache as apply_rope_with_cos_sin_cache
from .rope import (
    apply_rope_with_cos_sin_cache_inplace as apply_rope_with_cos_sin_cache_inplace,
)
from .sampling import chain_speculative_sampling as chain_speculative_sampling
from .sampling import min_p_sampling_from_probs as min_p_sampling_from_probs
from .sampling import sampling_from_logits as sampling_from_logits
from .sampling import sampling_from_probs as sampling_from_probs
from .sampling import softmax as softmax
from .sampling import top_k_mask_logits as top_k_mask_logits
from .sampling import top_k_renorm_probs as top_k_renorm_probs
from .sampling import top_k_sampling_from_probs as top_k_sampling_from_probs
from .sampling import (
    top_k_top_p_sampling_from_logits as top_k_top_p_sampling_from_logits,
)
from .sampling import top_k_top_p_sampling_from_probs as top_k_top_p_sampling_from_probs
from .sampling import top_p_renorm_probs as top_p_renorm_probs
from .sampling import top_p_sampling_from_probs as top_p_sampling_from_probs
from .sparse import BlockSparseAttentionWrapper as BlockSparseAttentionWrapper
from .sparse import (
    VariableBlockSparseAttentionWrapper as VariableBlockSparseAttentionWrapper,
)
from .utils import next_positive_power_of_2 as next_positive_power_of_2

__version__ = "0.3.1+mi355x.r2"
