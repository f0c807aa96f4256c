// What the two planners that run on the GPU (decode_plan_device.hip, prefill_plan_device.hip) share: the workgroup
// shape, the clamp of a device-resident length to its block-table row, and the CSR page table cut from that row.
#pragma once
#include "common.h"

namespace fi {

constexpr int kPlanThreads = 256;
constexpr int kPlanWaves = kPlanThreads / 64;

// tokens of request b the plan covers: the length clamped to what its block-table row can hold (a negative one: 0)
__device__ __forceinline__ int32_t planned_kv_len(const int32_t* seq_lens, int b, int32_t max_blocks,
                                                  int32_t page_size) {
  return min(max(seq_lens[b], 0), max_blocks * page_size);
}
__device__ __forceinline__ uint32_t pages_holding(int32_t len, int32_t page_size) {
  return ((uint32_t)len + (uint32_t)page_size - 1) / (uint32_t)page_size;
}
// tokens in the last of the np pages that hold len tokens; 0 for a request without a page
__device__ __forceinline__ int32_t last_page_tokens(int32_t len, int32_t np, int32_t page_size) {
  return np > 0 ? len - (np - 1) * page_size : 0;
}
// entry j of block-table row b to its place in `indices`, when the request has that many pages.  The store is bounded
// by indptr[b] + j < indptr[batch] <= batch * max_blocks.
__device__ __forceinline__ void compact_page_id(const int32_t* block_tables, int64_t block_tables_stride,
                                                const int32_t* indptr, int32_t* indices, int b, int j) {
  const int32_t begin = indptr[b];
  if (j < indptr[b + 1] - begin) indices[begin + j] = block_tables[(int64_t)b * block_tables_stride + j];
}

}  // namespace fi
