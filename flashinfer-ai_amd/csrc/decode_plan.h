// What the host decode planner (decode.hip) and the device decode planner (decode_plan_device.hip) share: the
// launch shape a batch-decode plan is cut for.  Everything here is known on the host without reading a length.
#pragma once
#include "common.h"

namespace fi {

struct DecodeGridShape {
  uint32_t gdy;       // waves per work-list entry: kv heads x the head tiles of the kernel a plain run() gets
  uint32_t max_grid;  // waves the plan fills: max_grid_hint when positive, else CUs x resident waves
};

// The kernel a plain run() gets (no RoPE, plain logits, strides that fit) decides gdy; see fi_batch_decode_plan.
DecodeGridShape decode_grid_shape(int num_qo_heads, int num_kv_heads, int head_dim, int page_size, int q_dtype,
                                  int kv_dtype, int max_grid_hint);

// a batch-decode kernel exists for the cache dtype and head_dim
bool decode_kernel_exists(int kv_dtype, int head_dim);

}  // namespace fi
