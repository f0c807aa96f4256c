// What the host MLA planner (mla.hip) and the device MLA planner (mla_plan_device.hip) share: the sizes a plan is cut
// for, the layout of the int workspace mla_paged_kernel reads, and the partial-state layout of the float workspace.
#pragma once
#include "common.h"

namespace fi {

constexpr int kMlaCkv = 512, kMlaKpe = 64, kMlaQK = kMlaCkv + kMlaKpe;
constexpr int kMlaRows = 16;                      // packed rows per work item
constexpr int kMlaTileKV = 64;                    // tokens per LDS tile
// resident workgroups per CU the planner fills: the kernel takes 256 arch + 165 accumulator registers per lane
// (-Rpass-analysis=kernel-resource-usage), one wave per SIMD, so one 4-wave workgroup per CU
constexpr int kMlaWgPerCu = 1;
constexpr int kMlaMinChunk = 256;                 // smallest kv chunk a split cuts (tokens)
constexpr int kMlaHeaderBytes = 64;               // int workspace: header, then merge indptr, then items

// int workspace header (int32 slots)
enum { kMlaHdrMagic = 0, kMlaHdrNumWork = 1, kMlaHdrItemsOff = 2, kMlaHdrSplit = 3 };
constexpr int32_t kMlaWsMagic = 0x4d4c4131;  // "MLA1"

// one work item (int32 x 8)
struct MlaItem {
  int32_t qo_start;   // first query token of the request (qo_indptr[b])
  int32_t row0;       // first packed row of the tile, within the request
  int32_t qo_len;
  int32_t kv_start, kv_end;  // the chunk [kv_start, kv_end)
  int32_t kv_len;
  int32_t page_base;  // kv_indptr[b]; a device plan: b * block_tables_stride, the request's block-table row
  int32_t chunk;      // chunk index within the request; -1: the request is not split (write o / lse directly)
};
static_assert(sizeof(MlaItem) == 32, "MlaItem layout");

// byte offset of the items: behind the header and the merge indptr [total_rows + 1]
inline int64_t mla_items_offset(int64_t total_rows) {
  return ceil_div<int64_t>(kMlaHeaderBytes + (total_rows + 1) * 4, 32) * 32;
}

// Partial-state layout in the float workspace, fixed by its size alone so that a captured run() keeps valid
// pointers across re-plans: lse entries first, then the 512-wide f32 rows.
inline int64_t mla_max_entries(size_t float_ws_bytes) {
  return (int64_t)(float_ws_bytes / (sizeof(float) * (kMlaCkv + 1))) / 4 * 4;
}
inline int64_t mla_v_offset(size_t float_ws_bytes) { return mla_max_entries(float_ws_bytes) * (int64_t)sizeof(float); }

}  // namespace fi
