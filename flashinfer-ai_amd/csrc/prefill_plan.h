// What the host prefill planner (prefill.hip) and the device prefill planner (prefill_plan_device.hip) share: the tile
// sizes a plan is cut for, the kv span of a request and the item budget of a launch.
#pragma once
#include "common.h"

namespace fi {

constexpr int kPlanTileQ = 128;  // packed query rows per work item (kTileQ of prefill_kernel.h)
constexpr int kPlanTileKV = 64;  // kv rows per tile; chunk sizes are multiples of it (kTileKV)

// keys a request's chunks are cut from.  Sliding window: a q tile only walks the keys from its first row's window
// start on (the kernel skips the rest), so chunks are cut from that span (ref: effective_kv_len_arr,
// scheduler.cuh:561-567)
__host__ __device__ inline int64_t kv_span(int64_t kv_len, int64_t qo_len, bool causal, int window_left) {
  const int64_t span = kv_len > 1 ? kv_len : 1;
  if (window_left < 0) return span;
  const int64_t walked = (int64_t)window_left + (causal ? kPlanTileQ : qo_len) + kPlanTileKV;
  return span < walked ? span : walked;
}

// resident workgroups (2 per CU) over the kv heads each item is launched for
// (ref: max_batch_size_if_split = max_grid_size / num_kv_heads, scheduler.cuh:718)
int64_t resident_items(int num_kv_heads);

}  // namespace fi
