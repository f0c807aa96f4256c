/*
 * fi_mi355.h -- C ABI of libfi_mi355.so, the MI355X (gfx950) implementation of FlashInfer's
 * batch paged-KV attention hot path (decode / prefill / cascade merge / page append), the fp8
 * groupwise (grouped) GEMM, the sampling operators, the norm / gated-activation operators, the MX quantisers with the
 * MXFP4-weight grouped GEMM, and the MoE layer built on it.
 *
 * Every entry point replaces one TVM-FFI export of the reference (FlashInfer v0.3.1); the export it
 * stands in for is cited as `ref: file:line` (paths relative to the reference checkout).  The
 * reference passes DLPack tensor views; this ABI passes the same information as plain device pointers,
 * element strides and sizes, so it can be bound from ctypes / cgo / JNI without torch types.
 *
 * Conventions
 *   - return value: 0 on success, non-zero on failure; fi_last_error() returns a thread-local message
 *     (the reference throws flashinfer::Error / TVM_FFI_ICHECK, ref: include/flashinfer/exception.h:23).
 *   - all tensors are borrowed; outputs are pre-allocated by the caller
 *     (ref: flashinfer/decode.py:1262-1275).
 *   - `stream` is a hipStream_t passed as void* (the reference takes the current torch stream,
 *     ref: csrc/tvm_ffi_utils.h:256-264).  No call synchronises the device.
 *   - strides are in ELEMENTS, not bytes (as paged_kv_t, ref: include/flashinfer/page.cuh:127-145).
 *   - log-sum-exp values are base 2 (ref: include/flashinfer/attention/state.cuh:45), and an empty
 *     KV range yields o = 0, lse = FI_NEG_INF (-5e4, ref: include/flashinfer/math.cuh:32).
 *   - attention sinks (the *_run_sinks entry points; ref: AttentionSink, flashinfer/jit/attention/variants.py:17-53):
 *     `sinks` is f32 [num_qo_heads] on the device, one logit per head in natural-log units, NOT multiplied by
 *     sm_scale.  Row probabilities become p_j = exp(s_j) / (sum_k exp(s_k) + exp(sink_h)) over the final logits s
 *     (after sm_scale, soft cap, mask and window); the sink has no value vector.  The result is the state (o, lse)
 *     merged with (0, sink_h * log2(e)), and the returned lse includes the sink:
 *     lse' = log2(2^lse + 2^(sink_h * log2(e))).  Such a state must not be merged with others again.  What the
 *     reference does not pin: an empty KV range with a finite sink gives o = 0, lse = sink_h * log2(e);
 *     sink_h = -inf switches the sink off for that head (o and lse are bit for bit those of the run without sinks);
 *     an empty KV range with sink_h = -inf gives o = 0, lse = FI_NEG_INF.  sinks == NULL is the plain run.
 *
 * This file is also the source of the Python binding: flashinfer/_abi.py parses it at import into the ctypes
 * structures, prototypes and constants (there is no second copy to edit).  Keep declarations in the forms already
 * used here -- `typedef struct tag { ... } tag_t;` with scalar, pointer and struct-typed fields, `FI_API <ret>
 * fi_xxx(<params>);`, `#define FI_NAME <integer or float literal>`, enums with an explicit value for every
 * enumerator -- and no arrays, bit-fields, unions or function pointers: the parser refuses what it does not know.
 */
#ifndef FI_MI355_H_
#define FI_MI355_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FI_ABI_VERSION 2
#define FI_NEG_INF (-5.0e4f)

typedef void* fi_stream_t; /* hipStream_t */

#if defined(FI_BUILDING_LIB)
#define FI_API __attribute__((visibility("default")))
#else
#define FI_API
#endif

/* element types (ref: dtype dispatch in csrc/tvm_ffi_utils.h:70-200) */
enum fi_dtype {
  FI_DTYPE_F16 = 0,
  FI_DTYPE_BF16 = 1,
  FI_DTYPE_FP8_E4M3 = 2, /* OCP e4m3fn == torch.float8_e4m3fn */
  FI_DTYPE_FP8_E5M2 = 3,
  FI_DTYPE_F32 = 4
};

/* ref: flashinfer/utils.py:30-46 */
enum fi_pos_encoding_mode { FI_POS_NONE = 0, FI_POS_ROPE_LLAMA = 1, FI_POS_ALIBI = 2 };
enum fi_mask_mode { FI_MASK_NON_CAUSAL = 0, FI_MASK_CAUSAL = 1, FI_MASK_CUSTOM = 2, FI_MASK_MULTIITEMSCORING = 3 };

/* ------------------------------------------------------------------------------------------------
 * library / device information
 * ---------------------------------------------------------------------------------------------- */
FI_API const char* fi_last_error(void);
FI_API int fi_abi_version(void);
/* number of compute units the planner balances for (hipDeviceProp.multiProcessorCount of the current
 * device, or the switch FI_NUM_CUS when it is positive, or 256 when no device is visible). */
FI_API int fi_num_compute_units(void);
/* Set a kernel-choice switch of this process (names and values as the environment variables of INTEGRATION.md);
 * value == NULL returns the switch to what the environment gave it at load.  A set value wins over the environment.
 * Returns non-zero (fi_last_error) for an unknown name or a value that is not an integer. */
FI_API int fi_set_option(const char* name, const char* value);

/* ------------------------------------------------------------------------------------------------
 * Paged KV cache view.  ref: paged_kv_t, include/flashinfer/page.cuh:37-210.
 *   element offset of (page, head, entry, feat) = page*stride_page + head*stride_h + entry*stride_n + feat
 *   kv_len(b) = (indptr[b+1]-indptr[b]-1)*page_size + last_page_len[b]   (0 when the request has no page)
 * `indices == NULL` means the identity page table (page i of request 0 is physical page i): this is how
 * a dense [kv_len, H, D] tensor is addressed by fi_single_decode_run.
 * ---------------------------------------------------------------------------------------------- */
typedef struct fi_paged_kv {
  const void* k_data;
  const void* v_data;
  const int32_t* indptr;        /* [batch_size+1] device */
  const int32_t* indices;       /* [indptr[batch_size]] device */
  const int32_t* last_page_len; /* [batch_size] device */
  const int32_t* rope_pos_offset; /* optional [batch_size] device, NULL = 0 */
  int64_t stride_page, stride_n, stride_h;
  int32_t page_size;
  int32_t num_kv_heads;
  int32_t head_dim;
  int32_t batch_size;
  int32_t dtype; /* fi_dtype */
} fi_paged_kv_t;

/* ------------------------------------------------------------------------------------------------
 * Batch decode.  ref: BatchDecodeWithPagedKVCachePlan / Run, csrc/batch_decode.cu:39-79, 81-191;
 * planner DecodePlan, include/flashinfer/attention/scheduler.cuh:424-493.
 * ---------------------------------------------------------------------------------------------- */
#define FI_DECODE_PLAN_INFO_LEN 17
/* plan_info (int64[FI_DECODE_PLAN_INFO_LEN]); the reference's DecodePlanInfo has 10 entries
 * (scheduler.cuh:391-402); entries 0..9 keep their meaning, 10.. are ours. */
enum fi_decode_plan_slot {
  FI_DP_PADDED_BATCH_SIZE = 0, /* number of (request, kv-chunk) work items launched */
  FI_DP_V_OFFSET = 1,          /* byte offset of tmp_v in the float workspace */
  FI_DP_S_OFFSET = 2,          /* byte offset of tmp_s in the float workspace */
  FI_DP_REQUEST_INDICES_OFFSET = 3,
  FI_DP_KV_TILE_INDICES_OFFSET = 4,
  FI_DP_O_INDPTR_OFFSET = 5,
  FI_DP_BLOCK_VALID_MASK_OFFSET = 6,
  FI_DP_KV_CHUNK_SIZE_PTR_OFFSET = 7,
  FI_DP_ENABLE_CUDA_GRAPH = 8,
  FI_DP_SPLIT_KV = 9,
  FI_DP_KV_CHUNK_SIZE = 10, /* tokens per chunk */
  FI_DP_NUM_WORK = 11,      /* valid work items (<= padded) */
  FI_DP_BATCH_SIZE = 12,
  FI_DP_INT_BYTES_USED = 13,
  FI_DP_WINDOW_LEFT = 14,   /* sliding window the chunks were cut for (-1: none); run() must pass the same */
  FI_DP_MAGIC = 15,
  FI_DP_UNIFORM_CHUNKS = 16 /* n in {2, 4} when the plan is split, not a graph plan, has no planned window
                               (FI_DP_WINDOW_LEFT < 0) and EVERY request has exactly n chunks; else 0.  run() then
                               merges the chunks inside the decode launch where its kernel can */
};
#define FI_DECODE_PLAN_MAGIC 0x4649444543ll /* "FIDEC" */

/* Host-side planning.  Writes the work list into `pinned_int_ws` and, when `int_ws` is non-NULL,
 * enqueues ONE host-to-device copy of it on `stream` (ref: scheduler.cuh:488-491).  `int_ws == NULL`
 * plans on the host only (used by CPU tests).  `indptr_h` is the HOST copy of the page indptr.
 * `max_grid_hint` <= 0 lets the library size the grid from the device (CUs x resident waves).
 * `window_left` >= 0 (the reference passes it to plan too, csrc/batch_decode.cu:39-79): only the pages that
 * can intersect the window of the last token are partitioned into chunks; the pages before
 * max(0, (num_pages - 1) * page_size - window_left) / page_size are never read. */
FI_API int fi_batch_decode_plan(void* float_ws, size_t float_ws_bytes, void* int_ws, void* pinned_int_ws,
                         size_t int_ws_bytes, const int32_t* indptr_h, int32_t batch_size,
                         int32_t num_qo_heads, int32_t num_kv_heads, int32_t page_size,
                         int32_t enable_cuda_graph, int32_t head_dim, int32_t q_dtype,
                         int32_t kv_dtype, int32_t max_grid_hint, int32_t window_left,
                         int64_t* plan_info_out, fi_stream_t stream);

typedef struct fi_batch_decode_params {
  const void* q; /* [batch, num_qo_heads, head_dim], strides below */
  int64_t q_stride_n, q_stride_h;
  fi_paged_kv_t kv;
  void* o;    /* [batch, num_qo_heads, head_dim] contiguous, dtype = q dtype */
  float* lse; /* optional [batch, num_qo_heads] */
  const float* alibi_slopes;    /* [num_qo_heads], used when pos_encoding_mode == FI_POS_ALIBI */
  const int32_t* q_rope_offset; /* optional [batch]; NULL = kv_len-1 (ref: decode.cuh:445-450) */
  int32_t num_qo_heads;
  int32_t q_dtype;           /* FI_DTYPE_F16 / FI_DTYPE_BF16 */
  int32_t pos_encoding_mode; /* fi_pos_encoding_mode */
  int32_t window_left;       /* -1 = full */
  float logits_soft_cap;     /* 0 = off */
  float sm_scale;
  float rope_rcp_scale; /* 1/rope_scale */
  float rope_rcp_theta; /* 1/rope_theta */
} fi_batch_decode_params_t;

FI_API int fi_batch_decode_run(void* float_ws, size_t float_ws_bytes, void* int_ws, size_t int_ws_bytes,
                        const int64_t* plan_info, int32_t plan_info_len,
                        const fi_batch_decode_params_t* params, fi_stream_t stream);
/* fi_batch_decode_run with attention sinks (see Conventions; ref: flashinfer/jit/attention/variants.py:17-53, the
 * `sinks` argument of BatchDecodeWithPagedKVCacheWrapper.run, flashinfer/decode.py:1163-1374).  The sink is folded
 * once per output row, in the launch that writes the final output (the merge launch of a split plan): no extra
 * launch.  sinks == NULL is fi_batch_decode_run. */
FI_API int fi_batch_decode_run_sinks(void* float_ws, size_t float_ws_bytes, void* int_ws, size_t int_ws_bytes,
                              const int64_t* plan_info, int32_t plan_info_len,
                              const fi_batch_decode_params_t* params, const float* sinks, fi_stream_t stream);

/* Device-side planning: the plan of fi_batch_decode_plan(enable_cuda_graph = 1, window_left = -1), written by kernels
 * on `stream` from lengths that stay on the device.  No host read-back, no copy, no synchronisation: the call may be
 * captured in a graph together with the fi_batch_decode_run[_sinks] that follows it, and a replay plans again from
 * whatever `block_tables` and `seq_lens` hold then.  (The reference's plan-free decode entry,
 * trtllm_batch_decode_with_kv_cache, flashinfer/decode.py:2054-2071, takes the same two tensors.)
 *
 * The kernels also write the CSR page table run() addresses the cache through, into the int workspace at
 * csr_offsets_out[0..2] (byte offsets of indptr[batch+1], indices[batch * max_blocks], last_page_len[batch]):
 *   pages(b) = min(ceil(seq_lens[b] / page_size), max_blocks); indptr is their exclusive scan; indices holds the first
 *   pages(b) entries of row b, compacted; last_page_len[b] = len - (pages(b) - 1) * page_size, 0 for pages(b) == 0.
 * Row entries past pages(b) are never read.  A length beyond max_blocks * page_size (or below 0) is CLAMPED to that
 * range: it cannot be refused, the host never sees it.
 *
 * plan_info_out holds host-computed entries only: magic, ENABLE_CUDA_GRAPH = 1, WINDOW_LEFT = -1, UNIFORM_CHUNKS = 0,
 * the offsets, FI_DP_PADDED_BATCH_SIZE, and SPLIT_KV by the branch the host knows (batch * gdy >= max_grid: unsplit).
 * The list capacity of a split plan is max(max_grid / gdy, batch), what the host planner pads a graph plan to.  The
 * host grows its list beyond that when empty requests (one chunk each) make it longer; here the chunk search also
 * requires the list to fit, so such a batch gets longer chunks than the host would cut.  Every other batch, and every
 * batch without an empty request, gets the host's plan.
 * FI_DP_KV_CHUNK_SIZE and FI_DP_NUM_WORK are 0 here: both values exist on the device only, as two int32 at
 * FI_DP_KV_CHUNK_SIZE_PTR_OFFSET (tokens per chunk, which the decode kernels read through kv_chunk_size_ptr, then the
 * number of valid work items).
 * Errors (fi_last_error) before any launch: null tensors, batch_size <= 0, a workspace too small (the message states
 * the bytes needed), an unsupported head_dim / dtype. */
typedef struct fi_batch_decode_plan_device_params {
  const int32_t* block_tables; /* [batch_size, max_blocks] device, rows block_tables_stride elements apart */
  const int32_t* seq_lens;     /* [batch_size] device: kv tokens per request */
  int64_t block_tables_stride;
  void* int_ws; /* device: work list, then the CSR page table */
  size_t int_ws_bytes;
  void* float_ws; /* device: f32 partial states of a split plan (only sized here, run() writes it) */
  size_t float_ws_bytes;
  int32_t batch_size;
  int32_t max_blocks;
  int32_t page_size;
  int32_t num_qo_heads;
  int32_t num_kv_heads;
  int32_t head_dim;
  int32_t q_dtype;
  int32_t kv_dtype;
  int32_t max_grid_hint; /* <= 0: sized from the device, as fi_batch_decode_plan */
} fi_batch_decode_plan_device_params_t;

FI_API int fi_batch_decode_plan_device(const fi_batch_decode_plan_device_params_t* params, int64_t* plan_info_out,
                                       int64_t* csr_offsets_out, fi_stream_t stream);
/* The bytes fi_batch_decode_plan_device needs of the two workspaces for these params (the pointers and sizes in them
 * are not read): for callers that carve both regions out of one buffer.  Host arithmetic only. */
FI_API int fi_batch_decode_plan_device_workspace(const fi_batch_decode_plan_device_params_t* params,
                                                 size_t* int_ws_bytes_out, size_t* float_ws_bytes_out);

/* ------------------------------------------------------------------------------------------------
 * Single-request decode over a dense KV tensor.
 * ref: single_decode_with_kv_cache, csrc/single_decode.cu:33-104; decode.cuh:658-737.
 * k, v: [kv_len, num_kv_heads, head_dim] (NHD) or [num_kv_heads, kv_len, head_dim] (HND) described by
 * strides.  `tmp` holds split-KV partial states (the reference uses a 32 MB cache buffer,
 * flashinfer/decode.py:486).
 * ---------------------------------------------------------------------------------------------- */
typedef struct fi_single_decode_params {
  const void* q; /* [num_qo_heads, head_dim] */
  int64_t q_stride_h;
  const void* k;
  const void* v;
  int64_t kv_stride_n, kv_stride_h;
  void* o;    /* [num_qo_heads, head_dim] */
  float* lse; /* optional [num_qo_heads] */
  const float* alibi_slopes;
  int32_t kv_len, num_qo_heads, num_kv_heads, head_dim;
  int32_t q_dtype, kv_dtype;
  int32_t pos_encoding_mode;
  int32_t window_left;
  float logits_soft_cap, sm_scale, rope_rcp_scale, rope_rcp_theta;
} fi_single_decode_params_t;

FI_API int fi_single_decode_run(const fi_single_decode_params_t* params, void* tmp, size_t tmp_bytes,
                         fi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Attention-state merge (cascade).  ref: csrc/cascade.cu:23-57 (merge_state), 59-100
 * (merge_state_in_place), 102-... (merge_states); kernels include/flashinfer/attention/cascade.cuh.
 *   (v, s) (+) (v', s'):  m = max(s, s'); w = 2^(s-m); w' = 2^(s'-m);
 *   v_out = (w v + w' v') / (w + w');  s_out = m + log2(w + w')
 * v: [seq_len, num_heads, head_dim] f16/bf16/f32 contiguous; s: [seq_len, num_heads] f32.
 * ---------------------------------------------------------------------------------------------- */
FI_API int fi_merge_state(const void* v_a, const float* s_a, const void* v_b, const float* s_b,
                   void* v_merged, float* s_merged, int32_t seq_len, int32_t num_heads,
                   int32_t head_dim, int32_t dtype, fi_stream_t stream);
/* mask: optional uint8[seq_len]; rows with mask==0 keep (v, s) unchanged (cascade.cuh:86-116). */
FI_API int fi_merge_state_in_place(void* v, float* s, const void* v_other, const float* s_other,
                            const uint8_t* mask, int32_t seq_len, int32_t num_heads,
                            int32_t head_dim, int32_t dtype, fi_stream_t stream);
/* v: [seq_len, num_index_sets, num_heads, head_dim], s: [seq_len, num_index_sets, num_heads]. */
FI_API int fi_merge_states(const void* v, const float* s, void* v_merged, float* s_merged,
                    int32_t num_index_sets, int32_t seq_len, int32_t num_heads, int32_t head_dim,
                    int32_t dtype, fi_stream_t stream);
/* Ragged form used after split-KV (ref: VariableLengthMergeStates, cascade.cuh:686-736):
 * v: [nnz, num_heads, head_dim] of in_dtype, s: [nnz, num_heads]; row r merges entries
 * indptr[r]..indptr[r+1]; 0 entries -> zeros / FI_NEG_INF. */
FI_API int fi_variable_length_merge_states(const void* v, const float* s, const int32_t* indptr,
                                    void* v_merged, float* s_merged, int32_t seq_len,
                                    int32_t num_heads, int32_t head_dim, int32_t in_dtype,
                                    int32_t out_dtype, fi_stream_t stream);


/* ------------------------------------------------------------------------------------------------
 * Batch prefill / append attention over a paged KV cache.
 * ref: BatchPrefillWithKVCachePlan csrc/batch_prefill.cu:47-74, BatchPrefillWithPagedKVCacheRun
 * csrc/batch_prefill.cu:199-327; fp8: csrc/batch_prefill_fp8_sm90.cu:39-67, 81-185; planner
 * PrefillPlan include/flashinfer/attention/scheduler.cuh:694-795.
 * ---------------------------------------------------------------------------------------------- */
#define FI_PREFILL_PLAN_INFO_LEN 16
enum fi_prefill_plan_slot {
  FI_PP_PADDED_BATCH_SIZE = 0, /* work items launched (q tiles over all requests) */
  FI_PP_TOTAL_NUM_ROWS = 1,
  FI_PP_KV_CHUNK_SIZE_PTR_OFFSET = 2, /* int workspace: int32 chunk size the kernels read (rewritten by plan) */
  FI_PP_CTA_TILE_Q = 3,
  FI_PP_REQUEST_INDICES_OFFSET = 4,
  FI_PP_QO_TILE_INDICES_OFFSET = 5,
  FI_PP_KV_TILE_INDICES_OFFSET = 6, /* int workspace, valid when SPLIT_KV */
  FI_PP_MERGE_INDPTR_OFFSET = 7,    /* int workspace: [total_num_rows + 1] partial-state ranges per qo row */
  FI_PP_BATCH_SIZE = 8,
  FI_PP_KV_CHUNK_SIZE = 9,          /* tokens */
  FI_PP_V_OFFSET = 10,              /* float workspace: f32 partial outputs */
  FI_PP_S_OFFSET = 11,              /* float workspace: f32 partial lse */
  FI_PP_NUM_WORK = 12,              /* real work items (<= PADDED_BATCH_SIZE) */
  FI_PP_ENABLE_CUDA_GRAPH = 13,
  FI_PP_SPLIT_KV = 14,
  FI_PP_MAGIC = 15
};
#define FI_PREFILL_PLAN_MAGIC 0x4649505245ll /* "FIPRE" */

/* qo_indptr_h / kv_indptr_h: HOST [batch+1]; kv_len_arr_h: HOST [batch]. int_ws == NULL plans on the
 * host only.  The kv axis is split into chunks when the (request, q tile) items alone cannot fill the chip
 * (binary search of the chunk size as PrefillBinarySearchKVChunkSize, scheduler.cuh:101-130); partial states
 * then go to the float workspace and are merged by run().  fixed_split_size (tokens, > 0) fixes the chunk
 * size, disable_split_kv forbids splitting (batch-invariant results). */
FI_API int fi_batch_prefill_plan(void* float_ws, size_t float_ws_bytes, void* int_ws, void* pinned_int_ws,
                          size_t int_ws_bytes, const int32_t* qo_indptr_h, const int32_t* kv_indptr_h,
                          const int32_t* kv_len_arr_h, int32_t total_num_rows, int32_t batch_size,
                          int32_t num_qo_heads, int32_t num_kv_heads, int32_t page_size,
                          int32_t enable_cuda_graph, int32_t head_dim_qk, int32_t head_dim_vo,
                          int32_t causal, int32_t window_left, int32_t fixed_split_size,
                          int32_t disable_split_kv, int64_t* plan_info_out, fi_stream_t stream);

typedef struct fi_batch_prefill_params {
  const void* q; /* [nnz_qo, num_qo_heads, head_dim] */
  int64_t q_stride_n, q_stride_h;
  const int32_t* qo_indptr; /* [batch+1] device */
  fi_paged_kv_t kv;
  void* o;    /* [nnz_qo, num_qo_heads, head_dim] contiguous */
  float* lse; /* optional [nnz_qo, num_qo_heads] */
  const float* alibi_slopes;
  const float* scale_q; /* fp8 path: [num_qo_heads] (NULL = 1) */
  const float* scale_k; /* [num_kv_heads] */
  const float* scale_v; /* [num_kv_heads] */
  /* mask_mode CUSTOM (ref variants.cuh:57-86): bit (qo_idx * kv_len + kv_idx) of request r, little-endian
   * within bytes, starting at byte mask_indptr[r] of custom_mask (flashinfer.quantization.segment_packbits
   * layout, ref prefill.py:1203-1223, 1693-1706) */
  const uint8_t* custom_mask;
  const int32_t* mask_indptr; /* [batch+1] device, byte offsets */
  /* mask_mode MULTIITEMSCORING (ref: maybe_prefix_len_ptr / maybe_token_pos_in_items_ptr / maybe_max_item_len_ptr /
   * token_pos_in_items_len of paged_run, csrc/batch_prefill.cu:199-205, include/flashinfer/attention/prefill.cuh
   * :795-858): causal, and a query at position p >= prefix_len[b] sees only the prefix and the keys
   * kv_idx > p - token_pos_in_items[b][p - prefix_len[b]] (its own item).  max_item_len is accepted for
   * signature parity (the reference uses it to skip fully masked tiles) and may be NULL. */
  const uint32_t* prefix_len_ptr;         /* [batch] device */
  const uint16_t* token_pos_in_items_ptr; /* [batch, token_pos_in_items_len] device */
  const uint16_t* max_item_len_ptr;       /* [batch] device, optional */
  int32_t token_pos_in_items_len;
  int32_t num_qo_heads;
  int32_t q_dtype; /* f16 / bf16 / fp8_e4m3 (then kv must be fp8_e4m3 too) */
  int32_t o_dtype; /* f16 / bf16 */
  int32_t mask_mode; /* fi_mask_mode: NON_CAUSAL / CAUSAL / CUSTOM / MULTIITEMSCORING */
  int32_t pos_encoding_mode;
  int32_t window_left;
  float logits_soft_cap, sm_scale, rope_rcp_scale, rope_rcp_theta;
  /* bf16 queries only -- how the probabilities enter P.V (csrc/prefill_kernel.h, PMODE): 0 default = P.V on the f16
   * MFMA (P rounded to f16, V converted bf16 -> f16 while staged: exact for 2^-14 <= |v| < 65504, the result meets the
   * reference's 1e-3 bar); 1 = P as hi + lo bf16 halves on the bf16 MFMA (no range limit on V; ~25 % slower) -- for
   * caches that may hold |v| >= 65504 or many |v| < 6e-5; 2 = the default, explicitly; 3 = the reference's single bf16
   * rounding of P (prefill.cuh:962-985).  Ignored for other q dtypes. */
  int32_t bf16_pv_mode;
} fi_batch_prefill_params_t;

/* Ragged (non-paged) KV, ref BatchPrefillWithRaggedKVCacheRun csrc/batch_prefill.cu:76-197: pass the
 * [nnz_kv, H, D] tensors as a cache with page_size = 1, stride_page = stride_n, kv.indptr = the ragged
 * kv_indptr, kv.indices = NULL (identity) and kv.last_page_len = NULL (all pages full). */
FI_API int fi_batch_prefill_paged_run(void* float_ws, size_t float_ws_bytes, void* int_ws, size_t int_ws_bytes,
                               const int64_t* plan_info, int32_t plan_info_len,
                               const fi_batch_prefill_params_t* params, fi_stream_t stream);
/* fi_batch_prefill_paged_run (paged, or ragged K / V in the page_size = 1 form above) with attention sinks (see
 * Conventions; ref: flashinfer/jit/attention/variants.py:17-53, BatchAttentionWithAttentionSinkWrapper,
 * flashinfer/attention.py:201-275).  f16 / bf16 queries only: fp8 queries with sinks != NULL are refused before any
 * launch, and so is a head_dim_qk 192 / head_dim_vo 128 plan.  sinks == NULL is fi_batch_prefill_paged_run. */
FI_API int fi_batch_prefill_paged_run_sinks(void* float_ws, size_t float_ws_bytes, void* int_ws, size_t int_ws_bytes,
                                     const int64_t* plan_info, int32_t plan_info_len,
                                     const fi_batch_prefill_params_t* params, const float* sinks,
                                     fi_stream_t stream);

/* Device-side planning of a causal paged prefill: the plan of fi_batch_prefill_plan(enable_cuda_graph = 1, causal = 1)
 * written by kernels on `stream` from lengths that stay on the device, for the fi_batch_prefill_paged_run[_sinks] that
 * follows.  No host read-back, no copy, no synchronisation: both calls may be captured in one graph, and a replay plans
 * again from whatever `block_tables`, `seq_lens` and `cum_seq_lens_q` hold then.  (The reference's plan-free prefill
 * entry, trtllm_batch_context_with_kv_cache, flashinfer/prefill.py:3314-3334, takes the same tensors.)
 *
 * The rule is the host's graph-mode rule: 128-row q tiles over qo_len x group packed rows; span = max(kv_len, 1),
 * narrowed under a sliding window to window_left + 128 + 64; the chunk is 64 x the smallest n in
 * [2, ceil(max span / 64)] with sum(q_tiles x ceil(span / 64 n)) <= max_items, the range's upper end when none fits.
 * The work list is in request order (the host sorts requests by cost and interleaves wide and narrow items): per
 * request the q tiles from the last one down, per q tile the chunks upwards.
 *
 * The host knows one branch.  With T0 = ceil(total_num_rows x group / 128):
 *   T0 > max_items   no chunk size can fit, so the plan is unsplit: FI_PP_SPLIT_KV = 0, the kernels write the output
 *                    themselves, no merge is launched and the float workspace is not used (0 bytes).  List capacity
 *                    T0 + batch - 1.  (The host's graph plan routes such a batch through f32 partial states.)
 *   T0 <= max_items  FI_PP_SPLIT_KV = 1, merged with skip_empty as a host graph plan.  List capacity
 *                    max(max_items, T0 + batch - 1); partial states for max_items x (ceil(128 / group) + 1) entries.
 *
 * Device values are not trusted; every store is bounded by a host-known capacity:
 *   kv tokens of request b = clamp(seq_lens[b], 0, max_blocks x page_size), pages(b) = ceil(tokens / page_size);
 *   the kernels write their own qo_indptr[batch + 1] into the int workspace, qo_indptr[b] = max over j <= b of
 *   clamp(cum_seq_lens_q[j], 0, total_num_rows), and run() must be given THAT copy (params.qo_indptr), not the caller's.
 * csr_offsets_out[0..3]: byte offsets in the int workspace of the CSR indptr[batch + 1], indices[batch x max_blocks],
 * last_page_len[batch] (as fi_batch_decode_plan_device writes them) and of that qo_indptr.
 *
 * plan_info_out holds host-computed entries only: FI_PREFILL_PLAN_MAGIC, ENABLE_CUDA_GRAPH = 1, SPLIT_KV by the branch,
 * PADDED_BATCH_SIZE = the list capacity, TOTAL_NUM_ROWS = total_num_rows, the offsets.  FI_PP_KV_CHUNK_SIZE and
 * FI_PP_NUM_WORK are 0: both exist on the device only, as two int32 at FI_PP_KV_CHUNK_SIZE_PTR_OFFSET (tokens per
 * chunk, which the prefill kernels read through kv_chunk_size_ptr, then the number of real work items); entries of the
 * list past that number hold request -1.  merge_indptr has total_num_rows + 1 entries in both branches; rows past
 * qo_indptr[batch] get empty ranges, so the merge leaves them alone.
 * Errors (fi_last_error) before any launch: null tensors, batch_size <= 0, a workspace too small (the message states
 * the bytes needed), an unsupported head_dim / dtype pair. */
typedef struct fi_batch_prefill_plan_device_params {
  const int32_t* block_tables;   /* [batch_size, max_blocks] device, rows block_tables_stride elements apart */
  const int32_t* seq_lens;       /* [batch_size] device: kv tokens per request */
  const int32_t* cum_seq_lens_q; /* [batch_size + 1] device: first query row of each request, then their end */
  int64_t block_tables_stride;
  void* int_ws; /* device: work list, merge_indptr, qo_indptr, scans, then the CSR page table */
  size_t int_ws_bytes;
  void* float_ws; /* device: f32 partial states of a split plan (only sized here, run() writes it) */
  size_t float_ws_bytes;
  int32_t batch_size;
  int32_t max_blocks;
  int32_t page_size;
  int32_t total_num_rows; /* rows of q and of the output */
  int32_t num_qo_heads;
  int32_t num_kv_heads;
  int32_t head_dim;
  int32_t q_dtype;  /* f16 / bf16 / fp8_e4m3 */
  int32_t kv_dtype; /* the q dtype, or fp8 under a 16-bit q */
  int32_t window_left;    /* < 0: none */
  int32_t max_items_hint; /* <= 0: 2 workgroups per CU over the kv heads, as fi_batch_prefill_plan */
} fi_batch_prefill_plan_device_params_t;

FI_API int fi_batch_prefill_plan_device(const fi_batch_prefill_plan_device_params_t* params, int64_t* plan_info_out,
                                        int64_t* csr_offsets_out, fi_stream_t stream);
/* The bytes fi_batch_prefill_plan_device needs of the two workspaces for these params (the pointers and sizes in them
 * are not read).  Host arithmetic only. */
FI_API int fi_batch_prefill_plan_device_workspace(const fi_batch_prefill_plan_device_params_t* params,
                                                  size_t* int_ws_bytes_out, size_t* float_ws_bytes_out);

/* Single-request prefill over dense K/V.  ref: csrc/single_prefill.cu, flashinfer/prefill.py:960-1194. */
typedef struct fi_single_prefill_params {
  const void* q; /* [qo_len, num_qo_heads, head_dim] */
  int64_t q_stride_n, q_stride_h;
  const void* k; /* [kv_len, H, D] (NHD) or [H, kv_len, D] (HND) by strides */
  const void* v;
  int64_t kv_stride_n, kv_stride_h;
  void* o;
  float* lse;
  const float* alibi_slopes;
  const float* scale_q;
  const float* scale_k;
  const float* scale_v;
  const uint8_t* custom_mask; /* mask_mode CUSTOM: packed [qo_len * kv_len] bits, little-endian */
  int32_t qo_len, kv_len, num_qo_heads, num_kv_heads, head_dim;
  int32_t q_dtype, kv_dtype, o_dtype;
  int32_t mask_mode, pos_encoding_mode, window_left;
  float logits_soft_cap, sm_scale, rope_rcp_scale, rope_rcp_theta;
  int32_t bf16_pv_mode; /* as fi_batch_prefill_params_t.bf16_pv_mode */
} fi_single_prefill_params_t;

FI_API int fi_single_prefill_run(const fi_single_prefill_params_t* params, void* tmp, size_t tmp_bytes,
                          fi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Prefill with head_dim_qk 192 / head_dim_vo 128 (DeepSeek-style MLA in its non-absorbed form: prefill and
 * chunked prefill), ragged or single-request K / V, f16 or bf16.  ref: the FA2 prefill kernels at
 * (HEAD_DIM_QK, HEAD_DIM_VO) = (192, 128), flashinfer/aot.py:568.
 * K and V have separate head dims and separate strides (v may be a view into a fused projection output).
 * Plain logits only: mask_mode NON_CAUSAL / CAUSAL, window_left, sm_scale; q / k / v / o of one 16-bit
 * dtype.  fp8, pos_encoding_mode != NONE, logits_soft_cap > 0, custom masks and multi-item scoring are
 * refused.  Partial states of a split kv axis are head_dim_vo wide and merged by run().
 * ---------------------------------------------------------------------------------------------- */
/* plan_info[FI_PP_MAGIC] of a fi_batch_prefill_plan made with head_dim_qk 192 / head_dim_vo 128: only
 * fi_batch_prefill_qkvo_run takes such a plan, and it takes no other */
#define FI_PREFILL_QKVO_PLAN_MAGIC 0x4649514b564fll /* "FIQKVO" */

typedef struct fi_prefill_qkvo_params {
  const void* q; /* [rows, num_qo_heads, head_dim_qk] */
  int64_t q_stride_n, q_stride_h;
  const void* k; /* [kv rows, num_kv_heads, head_dim_qk] (NHD) or [num_kv_heads, kv rows, ...] (HND) by strides */
  int64_t k_stride_n, k_stride_h;
  const void* v; /* [kv rows, num_kv_heads, head_dim_vo] by its own strides */
  int64_t v_stride_n, v_stride_h;
  void* o;    /* [rows, num_qo_heads, head_dim_vo] contiguous */
  float* lse; /* optional [rows, num_qo_heads], base 2 */
  const int32_t* qo_indptr; /* batch run: [batch_size + 1] device; single run: unused */
  const int32_t* kv_indptr; /* batch run: [batch_size + 1] device, ragged K / V rows */
  int32_t batch_size;       /* batch run: as planned */
  int32_t qo_len, kv_len;   /* single run */
  int32_t num_qo_heads, num_kv_heads;
  int32_t head_dim_qk, head_dim_vo; /* 192, 128 */
  int32_t q_dtype, kv_dtype, o_dtype; /* all FI_DTYPE_F16 or all FI_DTYPE_BF16 */
  int32_t mask_mode;         /* FI_MASK_NON_CAUSAL / FI_MASK_CAUSAL */
  int32_t pos_encoding_mode; /* FI_POS_NONE */
  int32_t window_left;
  float logits_soft_cap; /* must be 0 */
  float sm_scale;
  int32_t bf16_pv_mode; /* as fi_batch_prefill_params_t.bf16_pv_mode */
} fi_prefill_qkvo_params_t;

/* Ragged batch run of a plan made by fi_batch_prefill_plan with head_dim_qk 192 / head_dim_vo 128. */
FI_API int fi_batch_prefill_qkvo_run(void* float_ws, size_t float_ws_bytes, void* int_ws, size_t int_ws_bytes,
                              const int64_t* plan_info, int32_t plan_info_len,
                              const fi_prefill_qkvo_params_t* params, fi_stream_t stream);
/* Single request over dense K / V (qo_len, kv_len); tmp as fi_single_prefill_run (split-kv scratch, may be NULL). */
FI_API int fi_single_prefill_qkvo_run(const fi_prefill_qkvo_params_t* params, void* tmp, size_t tmp_bytes,
                               fi_stream_t stream);

/* Bit packing of boolean masks (numpy.packbits semantics).  ref: csrc/quantization.cu,
 * include/flashinfer/quantization.cuh:29-126, Python flashinfer/quantization.py:57-153.
 *   x: n bytes, each 0 / non-zero;  y: ceil(n / 8) bytes;  bitorder_little: 0 = "big", 1 = "little".
 * Segment form: segment i is x[in_indptr[i] : in_indptr[i+1]], packed into
 * y[out_indptr[i] : out_indptr[i+1]] with out_indptr[i+1] - out_indptr[i] = ceil(len_i / 8) (both int32
 * device arrays of batch + 1 entries; y_bytes = out_indptr[batch], passed by the host for the launch). */
FI_API int fi_packbits(const uint8_t* x, int64_t n, int32_t bitorder_little, uint8_t* y, fi_stream_t stream);
FI_API int fi_segment_packbits(const uint8_t* x, const int32_t* in_indptr, const int32_t* out_indptr,
                               int32_t batch, int64_t y_bytes, int32_t bitorder_little, uint8_t* y,
                               fi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * fp8 groupwise-scaled GEMM / grouped GEMM ("nt": D = A . B^T, B given as (n, k)).
 * ref: gemm_fp8_nt_groupwise csrc/gemm_sm100_binding.cu:23, csrc/gemm_groupwise_sm100.cu:89-120;
 * group_gemm_fp8_nt_groupwise csrc/group_gemm_sm100_binding.cu:34,
 * csrc/group_gemm_fp8_groupwise_sm100.cu:89-124; Python flashinfer/gemm.py:2321-2484, 2657-2811.
 *   a: (m | cum_m, k) fp8;  b: (n, k) | (G, n, k) fp8;  d: (m | cum_m, n) f16/bf16
 *   scale_k_major = 0 ("MN"): a_scale (k/128, m/gran_m), b_scale ([G,] k/128, n/128)
 *   scale_k_major = 1 ("K") : a_scale (m/gran_m, k/128), b_scale ([G,] n/128, k/128)
 *   m_indptr: int32 [G+1] on the DEVICE (ref: gemm.py:2689-2691; entries multiples of 4).
 * The reference's workspace and mma_sm arguments have no counterpart (no workspace is needed).
 * ---------------------------------------------------------------------------------------------- */
FI_API int fi_gemm_fp8_nt_groupwise(const void* a, const void* b, const void* a_scale, const void* b_scale,
                             void* d, int32_t m, int32_t n, int32_t k, int32_t gran_m, int32_t gran_n,
                             int32_t gran_k, int32_t scale_k_major, int32_t a_dtype, int32_t b_dtype,
                             int32_t d_dtype, fi_stream_t stream);
FI_API int fi_group_gemm_fp8_nt_groupwise(const void* a, const void* b, const void* a_scale,
                                   const void* b_scale, void* d, const int32_t* m_indptr,
                                   int32_t num_groups, int32_t cum_m, int32_t n, int32_t k,
                                   int32_t gran_m, int32_t gran_n, int32_t gran_k, int32_t scale_k_major,
                                   int32_t a_dtype, int32_t b_dtype, int32_t d_dtype, fi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Page-table operations.  ref: append_paged_kv_cache csrc/flashinfer_page_binding.cu:36, csrc/page.cu,
 * include/flashinfer/page.cuh:258-284, 345-411; get_batch_indices_positions flashinfer/page.py:169-221.
 *   positions[i] = i + seq_lens[b] - append_indptr[b+1]   for append_indptr[b] <= i < append_indptr[b+1]
 *   append: K/V row i (shape [nnz, num_kv_heads, head_dim], element strides given) is written at
 *           page kv.indices[kv.indptr[b] + pos / page_size], entry pos % page_size.
 * `kv->k_data` / `kv->v_data` are WRITTEN by fi_append_paged_kv_cache; kv->last_page_len is unused.
 * ---------------------------------------------------------------------------------------------- */
FI_API int fi_get_batch_indices_positions(const int32_t* append_indptr, const int32_t* seq_lens,
                                   int32_t batch_size, int32_t nnz, int32_t* batch_indices,
                                   int32_t* positions, fi_stream_t stream);
FI_API int fi_append_paged_kv_cache(const void* append_key, const void* append_value, int64_t k_stride_n,
                             int64_t k_stride_h, int64_t v_stride_n, int64_t v_stride_h,
                             const int32_t* batch_indices, const int32_t* positions, int32_t nnz,
                             const fi_paged_kv_t* kv, fi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Block-sparse index plumbing (csrc/sparse.hip).  ref: the torch expansion of
 * VariableBlockSparseAttentionWrapper.plan, flashinfer/sparse.py:929-974;
 * BlockSparseIndicesToVectorSparseOffsetsKernel, include/flashinfer/page.cuh:287-302.
 *
 * A per-head block map `block_mask_map` [H, MB, NB] (one byte per entry, non-zero = selected) over column blocks
 * of `block_col_sz` [H, NB] tokens becomes a page table of `granule`-token pages; `granule` divides every column
 * size.  Head h owns tokens [h * kv_len, (h + 1) * kv_len), kv_len = sum_c block_col_sz[h, c] for every h; column
 * block c of head h starts at token h * kv_len + sum_{c' < c} block_col_sz[h, c'].
 *   row_pages[h * MB + i] = sum_c (mask[h, i, c] != 0) * block_col_sz[h, c] / granule
 *   fi_block_mask_to_page_indices: with kv_indptr [H * MB + 1] the exclusive scan of row_pages (device), row (h, i)
 *   writes, for its selected blocks in increasing c, the pages start / granule ... start / granule +
 *   block_col_sz / granule - 1 to kv_indices[kv_indptr[h * MB + i] ...].
 * Both refuse H * kv_len / granule >= 2^31 (page numbers are int32).  `num_pages` is kv_indptr[H * MB] as the host
 * knows it and `capacity` the number of int32 entries kv_indices holds: capacity < num_pages is refused before any
 * launch, and no row writes past its own end of kv_indptr or past `capacity`.
 *
 *   fi_block_sparse_indices_to_vector_sparse_offsets, for b < batch_size and pos < kv_lens[b]:
 *   vector_sparse_offsets[vector_sparse_indptr[b] + pos] =
 *       block_sparse_indices[block_sparse_indptr[b] + pos / block_size] * stride_block + (pos % block_size) * stride_n
 *   `num_indices` / `capacity` are the entries block_sparse_indices / vector_sparse_offsets hold: nothing is read or
 *   written past them.
 * ---------------------------------------------------------------------------------------------- */
FI_API int fi_block_mask_row_pages(const uint8_t* block_mask_map, const int32_t* block_col_sz, int32_t num_heads,
                                   int32_t num_block_rows, int32_t num_block_cols, int32_t granule, int64_t kv_len,
                                   int32_t* row_pages, fi_stream_t stream);
FI_API int fi_block_mask_to_page_indices(const uint8_t* block_mask_map, const int32_t* block_col_sz,
                                         const int32_t* kv_indptr, int32_t num_heads, int32_t num_block_rows,
                                         int32_t num_block_cols, int32_t granule, int64_t kv_len, int64_t num_pages,
                                         int64_t capacity, int32_t* kv_indices, fi_stream_t stream);
FI_API int fi_block_sparse_indices_to_vector_sparse_offsets(const int32_t* block_sparse_indices,
                                                            const int32_t* block_sparse_indptr,
                                                            int32_t* vector_sparse_offsets,
                                                            const int32_t* vector_sparse_indptr,
                                                            const int32_t* kv_lens, int64_t stride_block,
                                                            int64_t stride_n, int32_t batch_size, int32_t block_size,
                                                            int64_t num_indices, int64_t capacity,
                                                            fi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-head Latent Attention (absorbed form) over a paged cache.  ref: BatchMLAPagedAttentionWrapper,
 * flashinfer/mla.py:85-420; append_paged_mla_kv_cache flashinfer/page.py:250-298.
 *   one shared KV head; K = [ckv | kpe] (512 + 64 dims), V = ckv (512 dims)
 *   ckv cache: [pages, page_size, 512], kpe cache: [pages, page_size, 64] (element strides below)
 *   q_nope: [nnz_qo, num_heads, 512], q_pe: [nnz_qo, num_heads, 64]; o: [nnz_qo, num_heads, 512] contiguous
 *   causal: query qo_idx of a request sees keys kv_idx <= kv_len - qo_len + qo_idx
 * Packed row r of a request is (qo_idx = r / num_heads, head = r % num_heads); a work item is (request, tile of
 * 16 packed rows, kv chunk).  Only head_dim_ckv = 512, head_dim_kpe = 64 and q dtype == kv dtype (f16 / bf16).
 * A plan is cut from lengths alone: the planners take the compute dtype for both of their dtype fields, and an e4m3
 * cache or query is a matter of fi_batch_mla_run alone (q_fp8 / kv_fp8 of its params).
 * ---------------------------------------------------------------------------------------------- */
#define FI_MLA_PLAN_INFO_LEN 16
enum fi_mla_plan_slot {
  FI_MLA_NUM_WORK = 0,           /* work items */
  FI_MLA_GRID = 1,               /* workgroups launched (fixed for graph plans; the kernel strides over items) */
  FI_MLA_TOTAL_ROWS = 2,         /* qo_indptr[batch] * num_heads */
  FI_MLA_KV_CHUNK_SIZE = 3,      /* tokens */
  FI_MLA_SPLIT_KV = 4,           /* some request is cut into several chunks (then run() merges) */
  FI_MLA_ENABLE_CUDA_GRAPH = 5,  /* run() always launches kernel + merge */
  FI_MLA_NUM_HEADS = 6,
  FI_MLA_BATCH_SIZE = 7,
  FI_MLA_INT_BYTES_USED = 8,
  FI_MLA_MERGE_INDPTR_OFFSET = 9, /* int workspace: int32 [total_rows + 1], partial entries per packed row */
  FI_MLA_ITEMS_OFFSET = 10,       /* int workspace: int32 [num_work][8] work items (see csrc/mla.hip) */
  FI_MLA_NUM_ENTRIES = 11,        /* partial states written (f32 [entries, 512] + [entries]) */
  FI_MLA_V_OFFSET = 12,           /* float workspace: byte offset of the partial rows (lse entries start at 0) */
  FI_MLA_PAGE_SIZE = 13,
  FI_MLA_DTYPE = 14,
  FI_MLA_MAGIC = 15
};
#define FI_MLA_PLAN_MAGIC 0x46494d4c41ll /* "FIMLA" */

typedef struct fi_batch_mla_plan_params {
  void* int_ws;          /* device; NULL plans on the host only (CPU tests) */
  void* pinned_int_ws;   /* host; the plan is written here, then copied to int_ws on `stream` */
  size_t int_ws_bytes;
  size_t float_ws_bytes; /* size of the float workspace run() will get (partial states) */
  const int32_t* qo_indptr_h;  /* HOST [batch + 1] */
  const int32_t* kv_indptr_h;  /* HOST [batch + 1], pages */
  const int32_t* kv_len_arr_h; /* HOST [batch], tokens */
  int32_t batch_size, num_heads, head_dim_ckv, head_dim_kpe, page_size, causal;
  int32_t q_dtype, kv_dtype;
  int32_t enable_cuda_graph;
  int32_t fixed_split_size; /* > 0: kv chunk of this many tokens (rounded up to 64); 0: the planner's choice */
} fi_batch_mla_plan_params_t;

FI_API int fi_batch_mla_plan(const fi_batch_mla_plan_params_t* params, int64_t* plan_info_out, fi_stream_t stream);

typedef struct fi_batch_mla_params {
  const void* q_nope;
  int64_t q_nope_stride_n, q_nope_stride_h;
  const void* q_pe;
  int64_t q_pe_stride_n, q_pe_stride_h;
  const void* ckv;
  int64_t ckv_stride_page, ckv_stride_n;
  const void* kpe;
  int64_t kpe_stride_page, kpe_stride_n;
  const int32_t* kv_indices; /* device, the page table the plan's kv_indptr indexes */
  void* o;                   /* [nnz_qo, num_heads, 512] contiguous, q dtype */
  float* lse;                /* optional [nnz_qo, num_heads], base 2 */
  void* float_ws;
  size_t float_ws_bytes;
  void* int_ws;
  size_t int_ws_bytes;
  int32_t num_rows; /* nnz_qo * num_heads of the q tensors */
  int32_t num_heads, page_size, dtype, causal;
  float sm_scale;
  /* Storage types, 0 = the tensors hold `dtype` (f16 / bf16, the compute and output type, checked against the plan).
   * FI_DTYPE_FP8_E4M3: the tensors hold e4m3 bytes, upcast exactly to `dtype` while they are staged; their strides are
   * then multiples of 16 elements and their bases 16-byte aligned.  Offered: an fp8 cache with either query, and an
   * fp8 query with an fp8 cache and dtype = bf16.  Refused by name: an fp8 query with a 16-bit cache, and e5m2.
   * There is no scale in here: sm_scale is the full logit scale (the caller folds q_scale x k_scale into it) and the
   * caller applies v_scale to o. */
  int32_t q_fp8, kv_fp8;
  /* optional, device, one f32: the logit scale already multiplied by log2(e) (the reference's bmm1_scale_log2_tensor),
   * read by the kernel at run time in place of sm_scale x log2(e).  Only with an fp8 cache. */
  const float* sm_scale_log2_dev;
} fi_batch_mla_params_t;

FI_API int fi_batch_mla_run(const int64_t* plan_info, int32_t plan_info_len, const fi_batch_mla_params_t* params,
                            fi_stream_t stream);

/* Device-side planning: the int workspace of fi_batch_mla_plan(enable_cuda_graph = 1), written by kernels on `stream`
 * for qo_len = q_len_per_request in every request and kv_len = clamp(seq_lens[b], 0, max_blocks x page_size), from
 * lengths that stay on the device.  No host read-back, no copy, no synchronisation: the call may be captured in a graph
 * together with the fi_batch_mla_run that follows it, and a replay plans again from whatever `seq_lens` holds then.
 * (The reference's plan-free MLA entry, trtllm_batch_decode_with_kv_cache_mla, flashinfer/decode.py:2298-2315, takes
 * the same two tensors.)
 *
 * The header, the merge indptr [total_rows + 1] and the item list (request, then chunk, then row tile) are the host
 * planner's, by the host planner's chunk rule, with one field apart: there is no CSR page table, an item's page_base
 * is b x block_tables_stride, and run() is given kv_indices = block_tables.  Entries of a row past the request's
 * ceil(kv_len / page_size) pages are never read.  The list has the host-known capacity
 * max(max_items, batch x ceil(q_len_per_request x num_heads / 16)); items past the header's count are not written.
 * Behind the list the two kernels keep two scans of batch + 1 int32 each.
 *
 * plan_info_out holds host-known entries only: FI_MLA_PLAN_MAGIC, GRID = max_items, ENABLE_CUDA_GRAPH = 1 (run() always
 * merges), TOTAL_ROWS = batch x q_len_per_request x num_heads, NUM_HEADS, BATCH_SIZE, PAGE_SIZE, DTYPE, V_OFFSET,
 * INT_BYTES_USED (the list at its capacity, and the scans), the two offsets.  Decided on the device, and 0 here:
 * FI_MLA_NUM_WORK and FI_MLA_SPLIT_KV (header slots 1 and 3 of the int workspace), FI_MLA_KV_CHUNK_SIZE (in the items
 * only) and FI_MLA_NUM_ENTRIES (merge_indptr[total_rows]; never more than the float workspace holds).
 * Errors (fi_last_error) before any launch: null tensors, bad sizes, a workspace too small (the message states the bytes
 * needed), head dims other than 512 / 64, dtypes other than f16 / bf16 or differing. */
typedef struct fi_batch_mla_plan_device_params {
  const int32_t* block_tables; /* [batch_size, max_blocks] device, rows block_tables_stride elements apart */
  const int32_t* seq_lens;     /* [batch_size] device: kv tokens per request */
  int64_t block_tables_stride;
  void* int_ws; /* device: header, merge indptr, items, scans */
  size_t int_ws_bytes;
  void* float_ws; /* device: f32 partial states (only sized here, run() writes it); chunks grow until they fit */
  size_t float_ws_bytes;
  int32_t batch_size;
  int32_t max_blocks;
  int32_t page_size;
  int32_t num_heads;
  int32_t q_len_per_request; /* query tokens of every request; causal masks align them to the end of the keys */
  int32_t head_dim_ckv;
  int32_t head_dim_kpe;
  int32_t q_dtype;
  int32_t kv_dtype;
  int32_t max_items_hint; /* <= 0: one workgroup per CU (fi_num_compute_units), as fi_batch_mla_plan */
} fi_batch_mla_plan_device_params_t;

FI_API int fi_batch_mla_plan_device(const fi_batch_mla_plan_device_params_t* params, int64_t* plan_info_out,
                                    fi_stream_t stream);
/* The bytes fi_batch_mla_plan_device needs of the int workspace for these params (the pointers and sizes in them are not
 * read), and the least it needs of the float workspace: 0, a plan that cannot split is still correct.  Whatever more
 * the caller gives as float workspace lets the planner cut shorter chunks.  Host arithmetic only. */
FI_API int fi_batch_mla_plan_device_workspace(const fi_batch_mla_plan_device_params_t* params,
                                              size_t* int_ws_bytes_out, size_t* float_ws_bytes_out);

/* Append: row i of append_ckv [nnz, 512] / append_kpe [nnz, 64] goes to page
 * kv_indices[kv_indptr[batch_indices[i]] + positions[i] / page_size], entry positions[i] % page_size.
 * dtype: f16 / bf16 (72 16-byte chunks per token) or FI_DTYPE_FP8_E4M3 / FI_DTYPE_FP8_E5M2 (36); the rows are copied as
 * bytes.  Every row 16-byte aligned: strides multiples of 16 / sizeof(dtype) elements, bases 16-byte aligned. */
typedef struct fi_append_paged_mla_kv_params {
  const void* append_ckv;
  int64_t append_ckv_stride_n;
  const void* append_kpe;
  int64_t append_kpe_stride_n;
  const int32_t* batch_indices; /* [nnz] device */
  const int32_t* positions;     /* [nnz] device */
  void* ckv_cache;
  int64_t ckv_stride_page, ckv_stride_n;
  void* kpe_cache;
  int64_t kpe_stride_page, kpe_stride_n;
  const int32_t* kv_indices;
  const int32_t* kv_indptr;
  int32_t nnz, page_size, head_dim_ckv, head_dim_kpe, dtype;
} fi_append_paged_mla_kv_params_t;

FI_API int fi_append_paged_mla_kv_cache(const fi_append_paged_mla_kv_params_t* params, fi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Standalone rotary embedding (SURVEY.md 8f "next" row).  ref: apply_rope / apply_rope_pos_ids /
 * apply_llama31_rope* / apply_rope_pos_ids_cos_sin_cache in csrc/rope.cu, include/flashinfer/pos_enc.cuh:465-1070,
 * flashinfer/rope.py:321-1150.  One entry point: positions are explicit (fi_rope_positions_from_indptr
 * expands the (indptr, offsets) form), llama-3.1 scaling enters through smooth_a / smooth_b
 * (pos_enc.cuh:976-977; 0, 0 = plain RoPE), cos_sin_cache != NULL selects the table form.
 * q/k: [nnz, heads, head_dim] f16/bf16 with element strides; q_out/k_out may alias q/k (in place).
 * ---------------------------------------------------------------------------------------------- */
typedef struct fi_rope_params {
  const void* q;
  const void* k;
  void* q_out;
  void* k_out;
  const int32_t* pos_ids;     /* [nnz] device */
  const float* cos_sin_cache; /* optional [max_pos, rotary_dim] f32: cos half | sin half */
  int64_t q_stride_n, q_stride_h, k_stride_n, k_stride_h;
  int64_t qo_stride_n, qo_stride_h, ko_stride_n, ko_stride_h;
  int32_t nnz, num_q_heads, num_k_heads, head_dim, rotary_dim;
  int32_t interleave; /* 1: pairs (2i, 2i+1); 0: pairs (i, i + rotary_dim/2) */
  int32_t dtype;
  float rope_rcp_scale, rope_rcp_theta, smooth_a, smooth_b;
} fi_rope_params_t;

FI_API int fi_apply_rope_pos_ids(const fi_rope_params_t* params, fi_stream_t stream);
/* RoPE fused with the cache append ("fused RoPE-then-append"; the reference runs
 * apply_rope_pos_ids (csrc/rope.cu) and then append_paged_kv_cache (csrc/page.cu:25-120) -- two passes over k):
 * q is rotated into q_out as above; each rotated k row is written ONCE, into the paged cache at
 * (batch_indices[i], positions[i]) (page.cuh:272-275), and the v row is copied beside it.  params->k_out and
 * its strides are ignored; params->pos_ids are the rotation positions (normally == positions); the cache must
 * have k's dtype.  Bit-identical to the two calls it replaces. */
FI_API int fi_apply_rope_append_paged_kv_cache(const fi_rope_params_t* params, const void* append_value,
                                        int64_t v_stride_n, int64_t v_stride_h, const int32_t* batch_indices,
                                        const int32_t* positions, const fi_paged_kv_t* kv, fi_stream_t stream);
/* pos_ids[i] = offsets[b] + i - indptr[b] for indptr[b] <= i < indptr[b+1] (ref: pos_enc.cuh:540-575) */
FI_API int fi_rope_positions_from_indptr(const int32_t* indptr, const int32_t* offsets, int32_t batch_size,
                                  int32_t nnz, int32_t* pos_ids, fi_stream_t stream);

/* MLA: rotate the rope parts of q and k and quantise all four parts to fp8, in one launch.  ref: mla_rope_quantize_fp8,
 * flashinfer/rope.py:1154-1220, kernel include/flashinfer/pos_enc.cuh:345-460.
 *   q_rope [nnz, num_heads, 64], k_rope [nnz, 64], q_nope [nnz, num_heads, 512], k_nope [nnz, 512]: f16 / bf16 (dtype),
 *   last dimension contiguous, the other strides in elements and free (slices of 576-wide tensors are taken as they are)
 *   *_out: the same shapes in out_dtype (FI_DTYPE_FP8_E4M3 / FI_DTYPE_FP8_E5M2), with strides of their own
 *   cos_sin_cache: f32 [max_pos, 64], cosines in columns 0..31 and sines in 32..63; row pos_ids[i] rotates token i
 *   pos_ids: [nnz] int32, or int64 with pos_ids_int64 = 1
 * The rotation is done in f32 (interleave = 1: pair (2i, 2i+1), else pair (i, i + 32), both with cos[i], sin[i]), the
 * result times quant_scale_q / quant_scale_kv in f32, then converted round-to-nearest-even, saturating at +-448 (e4m3)
 * or +-57344 (e5m2).  The nope parts are scaled and converted only.  Input rows 16-byte aligned (strides multiples of 8
 * elements), output rows 8-byte aligned (strides multiples of 8 elements). */
typedef struct fi_mla_rope_quantize_params {
  const void* q_rope;
  const void* k_rope;
  const void* q_nope;
  const void* k_nope;
  void* q_rope_out;
  void* k_rope_out;
  void* q_nope_out;
  void* k_nope_out;
  const float* cos_sin_cache;
  const void* pos_ids;
  int64_t q_rope_stride_n, q_rope_stride_h, k_rope_stride_n, q_nope_stride_n, q_nope_stride_h, k_nope_stride_n;
  int64_t q_rope_out_stride_n, q_rope_out_stride_h, k_rope_out_stride_n;
  int64_t q_nope_out_stride_n, q_nope_out_stride_h, k_nope_out_stride_n;
  int32_t nnz, num_heads, rope_dim, nope_dim; /* rope_dim 64, nope_dim 512 */
  int32_t dtype, out_dtype, pos_ids_int64, interleave;
  float quant_scale_q, quant_scale_kv;
} fi_mla_rope_quantize_params_t;

FI_API int fi_mla_rope_quantize(const fi_mla_rope_quantize_params_t* params, fi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Sampling: logits -> probabilities -> token.  ref: csrc/flashinfer_sampling_binding.cu:20-82 (exports),
 * csrc/sampling.cu, csrc/renorm.cu, kernels include/flashinfer/sampling.cuh, Python flashinfer/sampling.py.
 * All rows are f32 [num_rows, vocab] contiguous; one workgroup works on one output row.  A per-row parameter
 * is `*_arr[row]` when the array is given (device, `param_len` entries, the index is clamped to it; `row` is the
 * row drawn from, i.e. indices[i] for output i, which is the output row itself without indices) and the scalar
 * `*_val` otherwise.  Filters are exact thresholds found by a radix select over the float bit pattern
 * (no sort, a fixed number of passes); a draw is an inverse-CDF draw over the kept entries with one uniform
 * number from Philox4x32-10 keyed by (seed, offset, output row).  Defined results for degenerate input: a row
 * without a positive finite entry gives token 0; top_k == 0 or top_k >= vocab and top_p >= 1 switch that filter
 * off; top_p <= 0 keeps the maximum only; NaN entries are never kept.  vocab is at most 2^22; top-p expects rows that
 * sum to about 1 (an entry counts as at most 2.0).
 * ---------------------------------------------------------------------------------------------- */
typedef struct fi_sampling_params {
  const float* probs;       /* [num_rows, vocab] probabilities (logits for fi_sampling_from_logits) */
  int32_t* samples;         /* [batch] out */
  const int32_t* indices;   /* optional [batch]: output row i draws from row indices[i] (clamped to num_rows) */
  const int32_t* top_k_arr; /* optional [param_len] */
  const float* top_p_arr;   /* optional [param_len]; min_p for fi_min_p_sampling_from_probs */
  int32_t top_k_val;
  float top_p_val;
  int32_t batch, num_rows, vocab, param_len;
  uint64_t philox_seed, philox_offset;
} fi_sampling_params_t;

/* ref: sampling_from_logits / sampling_from_probs, csrc/flashinfer_sampling_binding.cu:23-27, 64-66 */
FI_API int fi_sampling_from_logits(const fi_sampling_params_t* params, fi_stream_t stream);
FI_API int fi_sampling_from_probs(const fi_sampling_params_t* params, fi_stream_t stream);
/* ref: top_k / top_p / min_p / top_k_top_p _sampling_from_probs, csrc/flashinfer_sampling_binding.cu:29-45, 68-74.
 * fi_top_k_top_p_sampling_from_probs is the "joint" filter: the intersection of both sets. */
FI_API int fi_top_k_sampling_from_probs(const fi_sampling_params_t* params, fi_stream_t stream);
FI_API int fi_top_p_sampling_from_probs(const fi_sampling_params_t* params, fi_stream_t stream);
FI_API int fi_min_p_sampling_from_probs(const fi_sampling_params_t* params, fi_stream_t stream);
FI_API int fi_top_k_top_p_sampling_from_probs(const fi_sampling_params_t* params, fi_stream_t stream);

typedef struct fi_row_transform_params {
  const float* in;   /* [batch, vocab] */
  float* out;        /* [batch, vocab], may alias in */
  const int32_t* top_k_arr;
  const float* scalar_arr; /* top_p (renorm) or temperature (softmax), optional [param_len] */
  int32_t top_k_val;
  float scalar_val;
  int32_t batch, vocab, param_len;
} fi_row_transform_params_t;

/* out = softmax(in / temperature); rows may hold -inf.  ref: softmax, csrc/flashinfer_sampling_binding.cu:20-21, 62,
 * include/flashinfer/sampling.cuh:314-435 (the reference's workspace and enable_pdl have no counterpart). */
FI_API int fi_softmax(const fi_row_transform_params_t* params, fi_stream_t stream);
/* ref: top_p_renorm_probs / top_k_renorm_probs / top_k_mask_logits, csrc/flashinfer_sampling_binding.cu:47-54, 76-80,
 * include/flashinfer/sampling.cuh:1592-1850 */
FI_API int fi_top_p_renorm_probs(const fi_row_transform_params_t* params, fi_stream_t stream);
FI_API int fi_top_k_renorm_probs(const fi_row_transform_params_t* params, fi_stream_t stream);
FI_API int fi_top_k_mask_logits(const fi_row_transform_params_t* params, fi_stream_t stream);

/* ref: chain_speculative_sampling, csrc/flashinfer_sampling_binding.cu:56-59, 82, sampling.cuh:2059-2190.
 * Draft token i is accepted while u_i * p_draft < p_target; the first rejected position is redrawn from
 * relu(target - draft) (the bonus position from target alone), later positions are -1.  The counters are
 * ADDED to (accepted: as if every position were tested on its own; emitted: the accepted prefix). */
typedef struct fi_chain_speculative_params {
  const float* draft_probs;       /* [batch, n, vocab] */
  const int32_t* draft_token_ids; /* [batch, n] (clamped to the vocabulary) */
  const float* target_probs;      /* [batch, n + 1, vocab] */
  int32_t* output_token_ids;      /* [batch, n + 1] out */
  int32_t* output_accepted_token_num;      /* [batch] in/out */
  int32_t* output_emitted_draft_token_num; /* [batch] in/out */
  int32_t batch, num_speculative_tokens, vocab;
  uint64_t philox_seed, philox_offset;
} fi_chain_speculative_params_t;

FI_API int fi_chain_speculative_sampling(const fi_chain_speculative_params_t* params, fi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Normalisation and gated activations: the operators a decoder layer runs around attention.
 * ref: csrc/norm.cu:24-162, include/flashinfer/norm.cuh, csrc/flashinfer_norm_binding.cu,
 * flashinfer/activation.py:33-88, include/flashinfer/activation.cuh.
 * Tensors are f16 or bf16 (`dtype`), the weight has the tensors' dtype and all arithmetic is f32; the only 16-bit
 * rounding is the final store.  `hidden` (and `d`) go from 1 to 65536.  No entry point keeps host state, so all
 * of them may be captured into a graph.  An empty batch returns 0 without a launch.
 * ---------------------------------------------------------------------------------------------- */
#define FI_NORM_MAX_HIDDEN 65536

/* out = in * rsqrt(mean(in^2) + eps) * (weight_bias + weight) per row of `hidden` contiguous elements.
 * weight_bias is 0 for RMSNorm and 1 for the Gemma form (ref: norm.cuh:118, 405).  num_heads == 1 is the row form
 * over [batch, hidden] (one workgroup per row; *_stride_h are ignored); num_heads > 1 is the head form over
 * [batch, num_heads, hidden] (QK-norm, one wave per (token, head) row; ref: QKRMSNormKernel, norm.cuh:142-260).
 * Strides are in elements and at least `hidden`.  `out` may be `in`. */
typedef struct fi_rmsnorm_params {
  const void* in;
  const void* weight; /* [hidden] */
  void* out;
  int32_t batch, num_heads, hidden;
  int64_t in_stride_n, in_stride_h, out_stride_n, out_stride_h;
  float eps, weight_bias;
  int32_t dtype;
} fi_rmsnorm_params_t;

FI_API int fi_rmsnorm(const fi_rmsnorm_params_t* params, fi_stream_t stream);

/* In place on both tensors (ref: FusedAddRMSNormKernel, norm.cuh:264-355): s = float(input) + float(residual);
 * residual = T(s); input = T(s * rsqrt(mean(s^2) + eps) * (weight_bias + weight)), the sum of squares and the output
 * taken from the unrounded f32 s.  input and residual must not overlap. */
typedef struct fi_fused_add_rmsnorm_params {
  void* input;    /* [batch, hidden] in/out */
  void* residual; /* [batch, hidden] in/out */
  const void* weight;
  int32_t batch, hidden;
  int64_t input_stride, residual_stride;
  float eps, weight_bias;
  int32_t dtype;
} fi_fused_add_rmsnorm_params_t;

FI_API int fi_fused_add_rmsnorm(const fi_fused_add_rmsnorm_params_t* params, fi_stream_t stream);

enum fi_activation { FI_ACT_SILU = 0, FI_ACT_GELU = 1, FI_ACT_GELU_TANH = 2 };

/* out[t, j] = act(in[t, j]) * in[t, d + j]; in [tokens, 2 d] and out [tokens, d] contiguous.
 * silu(x) = x / (1 + exp(-x)); gelu(x) = x/2 (1 + erf(x / sqrt 2)); gelu_tanh(x) = x/2 (1 + tanh(0.79788456
 * (x + 0.044715 x^3))) (ref: flashinfer/activation.py:33-52). */
typedef struct fi_act_and_mul_params {
  const void* in;
  void* out;
  int64_t tokens;
  int32_t d;
  int32_t act; /* enum fi_activation */
  int32_t dtype;
} fi_act_and_mul_params_t;

FI_API int fi_act_and_mul(const fi_act_and_mul_params_t* params, fi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * MX (microscaling) operands: e4m3 / e5m2 / e2m1 values with one E8M0 scale byte (value 2^(byte - 127)) per 32
 * consecutive k elements of a row.  ref: mxfp8_quantize flashinfer/fp8_quantization.py:179-212,
 * csrc/nv_internal/tensorrt_llm/kernels/quantization.cuh:586-688; group_gemm_mxfp8_mxfp4_nt_groupwise
 * flashinfer/gemm.py:2814-2949, include/flashinfer/gemm/group_gemm_mxfp4_groupwise_sm100.cuh:54-90.
 * The entry points keep no host state and never synchronise (m_indptr stays on the device), so all may be captured
 * into a graph; an empty problem returns 0 without a launch.
 *
 * Scale layouts.  Linear: [rows, nkb] bytes, nkb = k blocks per row.  Swizzled "128x4" (quantization.cuh:649-688):
 * rows pad to 128 and k blocks to 4, and the byte of (row r, block kb) is at
 *   (r/128)*ceil(nkb/4)*512 + (kb/4)*512 + (r%32)*16 + ((r%128)/32)*4 + kb%4.
 * Grouped swizzled (the a_scale of the grouped GEMM; group_gemm_mxfp4_groupwise_sm100.cuh:66-68): the rows of group
 * g start at scale row sf_off(g) = (m_indptr[g] + g*127)/128*128 and are swizzled on their own from there; the tensor
 * has sf_off(G) = (cum_m + G*127)/128*128 rows.  The b_scale of group g starts at byte g * ceil(n/128)*128 * (k/32).
 * ---------------------------------------------------------------------------------------------- */
enum fi_mx_sf_layout { FI_MX_SF_LINEAR = 0, FI_MX_SF_SWIZZLED_128X4 = 1 };

/* q = e4m3(x * 2^-e), sf = e + 127 per block of 32, where e is the smallest integer in [-127, 127] with
 * 448 * 2^e >= amax (an all-zero block: e = -127, byte 0, q = 0).  The scaling is exact and the conversion rounds to
 * nearest even.  One deliberate pin: the reference multiplies amax by an approximate reciprocal of 448, so at amax
 * exactly 448 * 2^e its hardware may pick e + 1; here the compare is exact and such a block gets e.
 * input: f16 / bf16 [m, k], k % 32 == 0, row stride in elements (a multiple of 8, base 16-byte aligned).
 * q: [m, k_pad] e4m3 contiguous, k_pad = k rounded up to `alignment` (a multiple of 32); padded columns are 0.
 * sf: sf_layout linear [m, k_pad/32] or swizzled (rows padded to 128, blocks to 4); with m_indptr != NULL
 * (device, [num_groups + 1], ascending, 0 <= m_indptr[0], m_indptr[num_groups] <= m) the grouped swizzled layout of
 * sf_off(num_groups) rows with m as cum_m, which needs k_pad % 128 == 0 to be read by the GEMM; rows of no group (below
 * m_indptr[0], at or past m_indptr[num_groups]) get their q and no scale row.  EVERY byte of sf is written, padding as 0. */
typedef struct fi_mxfp8_quantize_params {
  const void* input;
  void* q;
  void* sf;
  const int32_t* m_indptr; /* optional, device */
  int64_t input_stride;
  int64_t sf_bytes; /* size of the sf buffer */
  int32_t m, k, alignment, num_groups;
  int32_t sf_layout; /* enum fi_mx_sf_layout */
  int32_t dtype;     /* FI_DTYPE_F16 / FI_DTYPE_BF16 */
} fi_mxfp8_quantize_params_t;

FI_API int fi_mxfp8_quantize(const fi_mxfp8_quantize_params_t* params, fi_stream_t stream);

/* d[r, j] = sum_k a[r, k] 2^(sa[r, k/32] - 127) * e2m1(b[g, j, k]) 2^(sb[g, j, k/32] - 127) for the rows r of group g
 * (m_indptr[g] <= r < m_indptr[g+1]); f32 accumulation, one round-to-nearest to the output dtype.
 *   a: (cum_m, k) e4m3 / e5m2;  b: (G, n, k/2) bytes, element k = 2i in the low nibble of byte i; e2m1 codes 0..7 are
 *   {0, .5, 1, 1.5, 2, 3, 4, 6}, bit 3 is the sign;  a_scale: grouped swizzled, at least sf_off(G) * k/32 bytes;
 *   b_scale: swizzled per group, G * ceil(n/128)*128 * k/32 bytes;  m_indptr: int32 [G+1] on the DEVICE, ascending,
 *   m_indptr[G] <= cum_m;  d: (cum_m, n) f16 / bf16 contiguous.  n % 8 == 0, k % 128 == 0.
 * Empty groups are legal; rows of d at or past m_indptr[G] are not written; padding bytes of the scale tensors are
 * never read.  Scale byte 255 (the E8M0 NaN) and non-finite inputs are unspecified.  No workspace. */
typedef struct fi_group_gemm_mxfp4_params {
  const void* a;
  const void* b;
  const void* a_scale;
  const void* b_scale;
  void* d;
  const int32_t* m_indptr;
  int64_t a_scale_bytes, b_scale_bytes; /* sizes of the scale buffers, checked on the host */
  int32_t num_groups, cum_m, n, k;
  int32_t a_dtype; /* FI_DTYPE_FP8_E4M3 / FI_DTYPE_FP8_E5M2 */
  int32_t d_dtype; /* FI_DTYPE_F16 / FI_DTYPE_BF16 */
} fi_group_gemm_mxfp4_params_t;

FI_API int fi_group_gemm_mxfp8_mxfp4_nt_groupwise(const fi_group_gemm_mxfp4_params_t* params, fi_stream_t stream);

/* Dense MXFP4 x MXFP4 matmul (csrc/mm_fp4.hip; ref: mm_fp4 with use_nvfp4=False, block_size=32, flashinfer/gemm.py
 * :2012-2160):  d[r, j] = alpha * sum_k e2m1(a[r, k]) 2^(sa[r, k/32] - 127) * e2m1(b[j, k]) 2^(sb[j, k/32] - 127),
 * f32 accumulation, alpha multiplied in f32, one round-to-nearest to the output dtype.
 *   a: (m, k/2) bytes, b: (n, k/2) bytes, both contiguous, element k = 2i in the low nibble of byte i;
 *   a_scale / b_scale: swizzled "128x4" E8M0 bytes of (m, k/32) resp. (n, k/32): at least ceil(m/128)*128 * k/32 resp.
 *   ceil(n/128)*128 * k/32 bytes;  alpha: one float on the DEVICE or NULL (= 1), read by the kernel;
 *   d: (m, n) f16 / bf16 contiguous.  n % 8 == 0, k % 128 == 0, k > 0.
 * a and b 16-byte, d 8-byte, scales and alpha 4-byte aligned.  Padding bytes of the scale tensors never reach d.  Scale
 * byte 255 (the E8M0 NaN) is unspecified.  Two kernels (few rows: weight streaming with k split over a workgroup's waves;
 * many rows: 128 x 128 LDS tiles), chosen by m or by the switch FI_MM_FP4_KERNEL; the result never depends on
 * scheduling.  No workspace, no host state, no synchronisation; m == 0 or n == 0 returns 0 without a launch. */
typedef struct fi_mm_mxfp4_params {
  const void* a;
  const void* b;
  const void* a_scale;
  const void* b_scale;
  const float* alpha; /* optional, device */
  void* d;
  int64_t a_scale_bytes, b_scale_bytes; /* sizes of the scale buffers, checked on the host */
  int32_t m, n, k;
  int32_t d_dtype; /* FI_DTYPE_F16 / FI_DTYPE_BF16 */
} fi_mm_mxfp4_params_t;

FI_API int fi_mm_mxfp4(const fi_mm_mxfp4_params_t* params, fi_stream_t stream);

/* MXFP4 quantiser (ref: fp4_quantize with sf_vec_size 32 and UE8M0 scales, flashinfer/fp4_quantization.py:525-587,
 * quantization.cuh:427-499).  code = e2m1(x * 2^-e), sf = e + 127 per block of 32, where e is the smallest integer in
 * [-127, 127] with 6 * 2^e >= amax (an all-zero block: e = -127, byte 0, codes 0).  The scaling is exact, nothing
 * saturates, and the conversion rounds to nearest with ties to even.  One deliberate pin, as for MXFP8: the reference
 * multiplies amax by an approximate reciprocal of 6, so at amax exactly 6 * 2^e its hardware may pick e + 1; here the
 * compare is exact and such a block gets e.  The reference ignores its global scale with UE8M0 scales; there is none
 * here.  The sign nibble of a value that rounds to zero is unspecified; NaN / Inf and magnitudes below 2^-126 are
 * outside the contract.
 * input: f16 / bf16 [num_groups * rows, k], k % 32 == 0, row stride in elements (a multiple of 8, base 16-byte
 * aligned); group g owns rows [g * rows, (g + 1) * rows).  num_groups = 1 is the plain 2-D case.
 * q: [num_groups * rows, k/2] bytes contiguous, element 2i in the low nibble of byte i (the b of the grouped GEMM).
 * sf: linear [num_groups * rows, k/32], or swizzled: every group on its own, rows padded to 128 and blocks to 4,
 * num_groups * ceil(rows/128)*128 * ceil(k/128)*4 bytes (the b_scale of the grouped GEMM when k % 128 == 0).
 * EVERY byte of sf is written, padding as 0.  No host state, no synchronisation; an empty problem returns 0. */
typedef struct fi_mxfp4_quantize_params {
  const void* input;
  void* q;
  void* sf;
  int64_t input_stride;
  int64_t sf_bytes; /* size of the sf buffer */
  int32_t num_groups, rows, k;
  int32_t sf_layout; /* enum fi_mx_sf_layout */
  int32_t dtype;     /* FI_DTYPE_F16 / FI_DTYPE_BF16 */
} fi_mxfp4_quantize_params_t;

FI_API int fi_mxfp4_quantize(const fi_mxfp4_quantize_params_t* params, fi_stream_t stream);

/* Linear scale bytes [num_groups, rows, cols] (contiguous) -> the swizzled layout, every group on its own:
 * num_groups * ceil(rows/128)*128 * ceil(cols/4)*4 bytes, EVERY one written, padding as 0 (ref: block_scale_interleave,
 * flashinfer/fp4_quantization.py:590-619).  output is 4-byte aligned. */
typedef struct fi_mx_sf_interleave_params {
  const void* input;
  void* output;
  int64_t output_bytes; /* size of the output buffer */
  int32_t num_groups, rows, cols;
} fi_mx_sf_interleave_params_t;

FI_API int fi_mx_sf_interleave(const fi_mx_sf_interleave_params_t* params, fi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Mixture-of-experts layer with MXFP8 activations and MXFP4 weights (csrc/moe.hip): the four stages around the two
 * launches of fi_group_gemm_mxfp8_mxfp4_nt_groupwise.  ref: trtllm_fp4_block_scale_moe, flashinfer/fused_moe/core.py
 * :1819-1948 (its MXFP8 x MXFP4 mode); routing methods core.py:62-76; the permutation is routing_reference with
 * padding 1, tests/moe/test_trtllm_gen_fused_moe.py:1083-1142; the activation compute_with_experts,
 * tests/moe/test_trtllm_cutlass_fused_moe.py:195-203.  The stages have no counterpart of their own in the reference,
 * which runs the layer as one call.
 *   route -> permute -> GEMM1 -> gated activation -> GEMM2 -> finalize
 * No entry point keeps host state, reads a device value on the host or synchronises: all may be captured into a graph.
 * Every buffer's size depends on shapes alone.  An empty problem (num_tokens == 0) returns 0 without a launch.
 * Tensors are contiguous.  Expert e is local iff local_expert_offset <= e < local_expert_offset + local_num_experts;
 * expanded index i = t * top_k + j is slot j of token t.
 * ---------------------------------------------------------------------------------------------- */
#define FI_MOE_MAX_EXPERTS 512
#define FI_MOE_MAX_TOP_K 8
#define FI_MOE_SORT_BLOCK 256 /* expanded indices ranked by one wave of the permutation (sizes its workspace) */

/* the reference's RoutingMethodType values of the methods provided (core.py:62-76): 0, 1, 4, 5 by fi_moe_route, 2 and 3
 * by fi_moe_route_sigmoid */
enum fi_moe_routing {
  FI_MOE_ROUTING_DEFAULT = 0,           /* softmax over all experts -> top-k */
  FI_MOE_ROUTING_RENORMALIZE = 1,       /* top-k -> softmax over the chosen logits */
  FI_MOE_ROUTING_DEEPSEEK_V3 = 2,       /* sigmoid -> + bias -> top groups by their top-2 sum -> top-k of those groups */
  FI_MOE_ROUTING_LLAMA4 = 3,            /* top-1 -> sigmoid */
  FI_MOE_ROUTING_RENORMALIZE_NAIVE = 4, /* softmax -> top-k -> divide by the sum of the chosen */
  FI_MOE_ROUTING_TOPK = 5               /* top-k, the weight is the logit itself */
};

/* Slot j of token t is the expert of the j-th largest logit; equal logits go to the lower expert index (softmax is
 * monotone, so the methods that take the top-k of the probabilities choose the same experts).  Weights are computed
 * in f32 and rounded once to bf16.  NaN logits count as -inf.  1 <= top_k <= min(8, num_experts), num_experts <= 512. */
typedef struct fi_moe_route_params {
  const void* logits;     /* [num_tokens, num_experts] f32 / bf16 */
  int32_t* topk_ids;      /* out [num_tokens, top_k] */
  uint16_t* topk_weights; /* out [num_tokens, top_k] bf16 */
  int32_t num_tokens, num_experts, top_k;
  int32_t method; /* enum fi_moe_routing */
  int32_t dtype;  /* FI_DTYPE_F32 / FI_DTYPE_BF16 */
} fi_moe_route_params_t;

FI_API int fi_moe_route(const fi_moe_route_params_t* params, fi_stream_t stream);

/* The two sigmoid routing methods (ref: csrc/trtllm_fused_moe_routing_deepseek.cu:45-210, noaux_tc_ref of
 * tests/moe/test_trtllm_gen_fused_moe.py:1145-1183; csrc/trtllm_fused_moe_routing_llama4.cu).  All arithmetic is f32,
 * weights are rounded once to bf16, a NaN logit counts as -inf.  With s[e] = sigmoid(logit[t, e]):
 *   FI_MOE_ROUTING_DEEPSEEK_V3: b[e] = s[e] + bias[e].  With n_group > 1 the experts [g * epg, (g + 1) * epg), epg =
 *     num_experts / n_group, are group g; a group's score is the sum of its two largest b, and the topk_group groups of
 *     the largest score (equal scores: the lower group) are kept.  With n_group 0 or 1 every expert is a candidate and
 *     topk_group is not read.  Slot j is the candidate of the j-th largest b (equal b: the lower expert), and
 *       w[j] = s[id_j] * routed_scaling_factor / (sum_j s[id_j] + 1e-20f).
 *     An expert of a dropped group is never chosen, whatever the signs of b.
 *   FI_MOE_ROUTING_LLAMA4: top_k == 1; the id is the largest logit's (equal logits: the lower expert), w = s[id].
 *     bias, n_group, topk_group and routed_scaling_factor are not read.
 * num_experts <= 512, 1 <= top_k <= 8; with groups: num_experts % n_group == 0, epg >= 2, n_group <= 64,
 * 1 <= topk_group <= n_group, top_k <= topk_group * epg; without: top_k <= num_experts.  One launch. */
typedef struct fi_moe_route_sigmoid_params {
  const void* logits;     /* [num_tokens, num_experts] f32 / bf16 */
  const void* bias;       /* [num_experts] f32 / bf16; may be NULL for FI_MOE_ROUTING_LLAMA4 only */
  int32_t* topk_ids;      /* out [num_tokens, top_k] */
  uint16_t* topk_weights; /* out [num_tokens, top_k] bf16 */
  int32_t num_tokens, num_experts, top_k;
  int32_t n_group, topk_group;
  float routed_scaling_factor;
  int32_t method;     /* FI_MOE_ROUTING_DEEPSEEK_V3 / FI_MOE_ROUTING_LLAMA4 */
  int32_t dtype;      /* of logits: FI_DTYPE_F32 / FI_DTYPE_BF16 */
  int32_t bias_dtype; /* of bias: FI_DTYPE_F32 / FI_DTYPE_BF16 */
} fi_moe_route_sigmoid_params_t;

FI_API int fi_moe_route_sigmoid(const fi_moe_route_sigmoid_params_t* params, fi_stream_t stream);

/* Sorts the expanded indices by local expert and gathers the MXFP8 rows into the grouped GEMM's row operand.
 *   m_indptr[g] = number of slots routed to a local expert below local_expert_offset + g      (G = local_num_experts)
 *   expanded_to_permuted[i] = m_indptr[g] + the number of i' < i routed to the same expert g; -1 for a non-local slot
 *   x_permuted[p] = x[i / top_k] and its scale bytes at scale row sf_off(g) + p - m_indptr[g] of the grouped swizzled
 *   layout (above), for p = expanded_to_permuted[i] >= 0
 * so within an expert the rows ascend by expanded index and experts follow one another without padding rows.  The
 * result is deterministic: counts per block of FI_MOE_SORT_BLOCK indices, a scan over the blocks, a stable rank inside
 * the block; no atomic decides a placement.  EVERY byte of sf_permuted (sf_off(G) rows with num_tokens * top_k as cum_m)
 * is written, padding as 0; rows of x_permuted at or past m_indptr[G] are not written.  Four launches.
 * packed != 0: the low 16 bits of a topk_ids entry are the expert, the high 16 bits the bf16 weight (ref: topk_ids of
 * trtllm_fp4_block_scale_routed_moe, core.py:1987-1990), copied to unpacked_weights when that is given.
 * workspace: int32, at least (ceil(n / FI_MOE_SORT_BLOCK) * G + n) * 4 bytes with n = num_tokens * top_k.
 * hidden % 128 == 0; x, x_permuted 16-byte aligned; x_sf, sf_permuted 4-byte aligned. */
typedef struct fi_moe_permute_params {
  const int32_t* topk_ids;        /* [num_tokens, top_k] */
  const void* x;                  /* [num_tokens, hidden] e4m3 */
  const void* x_sf;               /* [num_tokens, hidden / 32] E8M0 bytes, linear */
  int32_t* m_indptr;              /* out [local_num_experts + 1] */
  int32_t* expanded_to_permuted;  /* out [num_tokens * top_k] */
  void* x_permuted;               /* out [num_tokens * top_k, hidden] */
  void* sf_permuted;              /* out, grouped swizzled */
  uint16_t* unpacked_weights;     /* optional out [num_tokens, top_k] bf16, packed ids only */
  int32_t* workspace;
  int64_t sf_bytes, workspace_bytes; /* sizes of sf_permuted and workspace */
  int32_t num_tokens, top_k, hidden;
  int32_t local_expert_offset, local_num_experts;
  int32_t packed;
} fi_moe_permute_params_t;

FI_API int fi_moe_permute_mxfp8(const fi_moe_permute_params_t* params, fi_stream_t stream);

/* Gated activation between the two GEMMs, quantised to MXFP8 for the second.  For row r of group g (m_indptr[g] <= r <
 * m_indptr[g+1]) and column c < intermediate, with x1 = x[r, c] (the linear half) and x2 = x[r, intermediate + c] (the
 * gate), all in f32:
 *   gt = min(x2 + bias[g, intermediate + c], limit[g]);  l = clamp(x1 + bias[g, c], -limit[g], limit[g]) + beta[g]
 *   act = gt * sigmoid(alpha[g] * gt) * l
 * bias / alpha / beta / limit == NULL mean 0 / 1 / 0 / +inf.  q and sf follow the rule of fi_mxfp8_quantize (the same
 * device code, csrc/mx_quant.h) in the grouped swizzled layout: EVERY byte of sf (sf_off(num_groups) rows with cum_m)
 * is written, padding as 0; rows of q at or past m_indptr[num_groups] are not written.  intermediate % 128 == 0. */
typedef struct fi_moe_gated_act_params {
  const void* x;           /* [cum_m, 2 * intermediate] bf16 */
  const int32_t* m_indptr; /* [num_groups + 1] device */
  const float* bias;       /* optional [num_groups, 2 * intermediate] */
  const float* alpha;      /* optional [num_groups] */
  const float* beta;       /* optional [num_groups] */
  const float* limit;      /* optional [num_groups] */
  void* q;                 /* out [cum_m, intermediate] e4m3 */
  void* sf;                /* out, grouped swizzled */
  int64_t sf_bytes;        /* size of sf */
  int32_t cum_m, intermediate, num_groups;
} fi_moe_gated_act_params_t;

FI_API int fi_moe_gated_act_mxfp8(const fi_moe_gated_act_params_t* params, fi_stream_t stream);

/* out[t] = bf16(sum_j w[t, j] * (y[p(t, j)] + bias[g(t, j)])) over the slots with 0 <= p(t, j) =
 * expanded_to_permuted[t * top_k + j] < rows, accumulated in f32 in the order of j; a token without such a slot gets
 * zeros.  g is the group whose m_indptr range holds p; bias == NULL is 0 and then m_indptr may be NULL too.
 * hidden % 8 == 0; y, out and bias 16-byte aligned. */
typedef struct fi_moe_finalize_params {
  const void* y;                       /* [rows, hidden] bf16 */
  const uint16_t* weights;             /* [num_tokens, top_k] bf16 */
  const int32_t* expanded_to_permuted; /* [num_tokens * top_k] */
  const float* bias;                   /* optional [num_groups, hidden] */
  const int32_t* m_indptr;             /* [num_groups + 1] device, needed with bias */
  void* out;                           /* [num_tokens, hidden] bf16 */
  int32_t num_tokens, top_k, hidden, num_groups, rows;
} fi_moe_finalize_params_t;

FI_API int fi_moe_finalize(const fi_moe_finalize_params_t* params, fi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The same layer on DeepSeek's fp8 block-scale format, around two launches of fi_group_gemm_fp8_nt_groupwise in its
 * (1, 128, 128) "K" scale mode.  ref: trtllm_fp8_block_scale_moe, flashinfer/fused_moe/core.py:1742-1816.
 *   route -> permute (fp8 block) -> GEMM1 -> gated activation (fp8 block) -> GEMM2 -> finalize
 * fi_moe_route, fi_moe_route_sigmoid and fi_moe_finalize are the ones above.  Activations carry one f32 scale per row
 * and 128 columns; the block rule (csrc/fp8_block_quant.h) is
 *   amax = max |x| over the block;  s = max(amax / 448, 2^-126);  q = e4m3(clamp(x / s, -448, 448)), nearest even,
 * amax / 448 being the reference kernel's rule (csrc/trtllm_fused_moe_dev_kernel.cu:141-152); an all-zero block gets
 * s = 2^-126 and q = 0, and the clamp keeps a quotient one ulp above 448 off the NaN byte 0x7F.
 * ---------------------------------------------------------------------------------------------- */

/* fi_moe_permute_mxfp8 for fp8 block-scale activations: m_indptr and expanded_to_permuted are the same for the same
 * ids (the same three sorting launches), and for p = expanded_to_permuted[i] >= 0, t = i / top_k:
 *   x_permuted[p] = x[t];  scale_permuted[p, kb] = x_scale[kb * scale_stride_kb + t * scale_stride_t]
 * scale_permuted is [num_tokens * top_k, hidden / 128] row-major, the a_scale of the grouped GEMM in "K" mode.  The
 * scales of the input are read through both strides (in elements, >= 0): [hidden / 128, num_tokens] contiguous, the
 * reference's layout, has strides (num_tokens, 1), the transposed view of a [num_tokens, hidden / 128] tensor
 * (1, hidden / 128).  Rows of x_permuted at or past m_indptr[G] are not written; rows of scale_permuted there are
 * written as 1.0f, so that EVERY word of scale_permuted is written (the GEMM's power-of-two check reads them all).
 * Four launches.  workspace as fi_moe_permute_mxfp8.  hidden % 128 == 0; x, x_permuted 16-byte aligned. */
typedef struct fi_moe_permute_fp8_block_params {
  const int32_t* topk_ids;       /* [num_tokens, top_k] */
  const void* x;                 /* [num_tokens, hidden] e4m3 */
  const float* x_scale;          /* (hidden / 128) x num_tokens values by the two strides */
  int32_t* m_indptr;             /* out [local_num_experts + 1] */
  int32_t* expanded_to_permuted; /* out [num_tokens * top_k] */
  void* x_permuted;              /* out [num_tokens * top_k, hidden] */
  float* scale_permuted;         /* out [num_tokens * top_k, hidden / 128] */
  uint16_t* unpacked_weights;    /* optional out [num_tokens, top_k] bf16, packed ids only */
  int32_t* workspace;
  int64_t scale_stride_kb, scale_stride_t;
  int64_t workspace_bytes;
  int32_t num_tokens, top_k, hidden;
  int32_t local_expert_offset, local_num_experts;
  int32_t packed;
} fi_moe_permute_fp8_block_params_t;

FI_API int fi_moe_permute_fp8_block(const fi_moe_permute_fp8_block_params_t* params, fi_stream_t stream);

/* Plain SwiGLU between the two GEMMs, quantised by the block rule above.  For row r < m_indptr[num_groups] and column
 * c < intermediate, with x1 = x[r, c] (the linear half) and x2 = x[r, intermediate + c] (the gate), in f32:
 *   act = x2 * sigmoid(x2) * x1
 * q[r] and scale[r, c / 128] follow from act by the block rule.  scale is [cum_m, intermediate / 128] row-major.  Rows
 * at or past m_indptr[num_groups]: x is not read, q is not written, scale is 1.0f (EVERY word of scale is written).
 * Only m_indptr[num_groups] is read.  intermediate % 128 == 0; x 16-byte, q 8-byte aligned. */
typedef struct fi_moe_gated_act_fp8_block_params {
  const void* x;           /* [cum_m, 2 * intermediate] bf16 */
  const int32_t* m_indptr; /* [num_groups + 1] device */
  void* q;                 /* out [cum_m, intermediate] e4m3 */
  float* scale;            /* out [cum_m, intermediate / 128] */
  int32_t cum_m, intermediate, num_groups;
} fi_moe_gated_act_fp8_block_params_t;

FI_API int fi_moe_gated_act_fp8_block(const fi_moe_gated_act_fp8_block_params_t* params, fi_stream_t stream);

/* The block rule above on f16 / bf16 rows (csrc/fp8_block_quantize.hip): what feeds fi_moe_permute_fp8_block.
 * input: [m, k], k % 128 == 0, row stride in elements (a multiple of 8, base 16-byte aligned).
 * q: [m, k] e4m3 contiguous, 8-byte aligned.  scale: [k / 128, m] contiguous, the reference's layout of
 * hidden_states_scale.  No host state, no synchronisation; an empty problem returns 0 without a launch. */
typedef struct fi_fp8_quantize_1x128_params {
  const void* input;
  void* q;
  float* scale;
  int64_t input_stride;
  int32_t m, k;
  int32_t dtype; /* FI_DTYPE_F16 / FI_DTYPE_BF16 */
} fi_fp8_quantize_1x128_params_t;

FI_API int fi_fp8_quantize_1x128(const fi_fp8_quantize_1x128_params_t* params, fi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FI_MI355_H_ */
