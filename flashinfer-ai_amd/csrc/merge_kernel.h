// Attention-state merge kernels (cascade).  HBM-bound: every state is read once, one wave per
// (row, head); lanes stride over head_dim so each load instruction is a contiguous 128/256-byte row
// segment.  Operator (ref: include/flashinfer/attention/cascade.cuh:44-71, state.cuh:52-63):
//   (v, s) (+) (v', s'):  m = max(s, s');  w = 2^(s-m), w' = 2^(s'-m)
//   v <- (w v + w' v') / (w + w'),  s <- m + log2(w + w')
//
// Empty states.  A state that saw no key comes in two encodings, both with v = 0:
//   * s = FI_NEG_INF (-5e4): what every attention kernel here writes for a chunk, row or request without a key -- the
//     partial states of split-KV decode (decode_kernel.h, decode_mfma_kernel.h, decode_mfma16_kernel.h), prefill
//     (prefill_kernel.h, prefill_fp8_kernel.h, prefill_qkvo_kernel.h) and MLA (mla.hip), and their final (o, lse):
//     l = 0 there, so inv = 0, v = acc * 0 = 0 and s = FI_NEG_INF.  An empty (row, chunk) slot that a merge
//     reads is written like any other; stale workspace bytes are never a state (tests/test_unowned_memory_gpu.py runs
//     every split path on a workspace of NaN bytes).
//   * s = -inf: what the reference's callers pass for a level that holds nothing.
// Both carry weight 2^(s - m) = 0 next to a live state.  merge_n_* turns a row of nothing but empty states into
// (0, FI_NEG_INF); merge_2 keeps the encoding it was given: (0, -inf) for two -inf states, (0, FI_NEG_INF + 1) for two
// FI_NEG_INF states -- either merges with a live state to that live state.
#pragma once
#include "common.h"

namespace fi {

constexpr int kMergeThreads = 256;
constexpr int kMergeWaves = kMergeThreads / 64;
constexpr int kMergeMaxPerLane = 8;  // head_dim <= 512

struct MergeNParams {
  const void* v;         // states
  const float* s;
  const int32_t* indptr;  // ragged: row r owns entries indptr[r]..indptr[r+1]; NULL: fixed n
  void* v_out;
  float* s_out;
  int32_t n_fixed;  // entries per row when indptr == NULL; layout [row, n, H, D]
  int32_t seq_len, num_heads, head_dim;
  int32_t in_dtype, out_dtype;
  int32_t skip_empty;  // rows without entries are left untouched (padding rows of a fixed-shape launch)
  // attention sinks, f32 [num_heads] natural-log logits (NULL: none): the merge of the split-KV partial states of a
  // run with sinks folds them (fold_sink, common.h), once per output row; a row of empty partials becomes
  // (0, sink_log2).  NULL everywhere else.
  const float* sinks;
};

struct Merge2Params {
  const void* v_a;
  const float* s_a;
  const void* v_b;
  const float* s_b;
  void* v_out;
  float* s_out;
  const uint8_t* mask;  // optional per-row; 0 = keep (v_a, s_a)
  int32_t seq_len, num_heads, head_dim, dtype;
};

hipError_t launch_merge_n(const MergeNParams& p, hipStream_t stream);
hipError_t launch_merge_2(const Merge2Params& p, hipStream_t stream);

}  // namespace fi
