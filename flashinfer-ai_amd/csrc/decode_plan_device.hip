// Batch decode: the planner that runs on the GPU (fi_batch_decode_plan_device).
//
// It writes what fi_batch_decode_plan(enable_cuda_graph = 1) writes -- request_indices, kv_tile_indices, o_indptr, the
// kv-chunk-size slot, block_valid_mask -- by the same rule (estimate_decode_work, decode.hip; the list's fixed capacity
// is one more condition of the chunk search, which only empty requests can make bite), plus the CSR page table the
// decode kernels address the cache through, from a dense block table and lengths that never leave the device.
// Two launches, both shaped by host-known values only:
//   decode_plan_scan_kernel   one workgroup: pages per request, their maximum, the chunk search (one block reduction
//                             per round of the bisection, <= 32 rounds), the scans for indptr and o_indptr
//   decode_plan_fill_kernel   fixed grid: the work list and its mask from o_indptr, the page ids compacted by indptr
// Plain vector loads and stores; no atomics; nothing is read back.
#include <algorithm>

#include "decode_plan.h"
#include "plan_device.h"

namespace fi {

struct DevicePlanParams {
  // work list (fi_decode_plan_slot offsets of the int workspace)
  int32_t* request_indices;    // [padded]
  int32_t* kv_tile_indices;    // [padded]
  int32_t* o_indptr;           // [batch + 1]
  int32_t* chunk_slot;         // [2]: tokens per chunk, valid work items
  uint8_t* block_valid_mask;   // [padded], null for an unsplit plan
  PlanPageTable csr;
  PlanRequests req;   // in front of the other scalars (plan_device.h)
  int32_t padded;     // capacity of the work list
  int32_t split;      // the host-known branch: batch * gdy < max_grid
  uint32_t gdy, max_grid;
  int32_t list_blocks;  // fill kernel: workgroups that write the work list; the rest compact page ids
};

__global__ __launch_bounds__(kPlanThreads) void decode_plan_scan_kernel(const DevicePlanParams p) {
  __shared__ uint32_t red[kPlanWaves];
  __shared__ int32_t wave_tot[2][kPlanWaves];
  const int tid = threadIdx.x;
  const int B = p.req.batch;

  // the longest request's pages and the requests without a page, in one pass over the lengths
  uint32_t max_pages = 0, empty = 0;
  for (int b = tid; b < B; b += kPlanThreads) {
    const uint32_t np = p.req.pages(b);
    max_pages = max(max_pages, np);
    empty += np == 0;
  }
  max_pages = block_reduce<kPlanWaves, RedMax>(max_pages, red);
  empty = block_reduce<kPlanWaves, RedSum>(empty, red);

  // estimate_decode_work (decode.hip): whole requests when they fill the grid, else smallest_fitting over
  // [max(128 / page_size, 1), max_pages].
  //
  // The list has a host-known capacity, padded = max(max_grid / gdy, batch), where the host planner grows its list
  // to the entries it counted.  Only empty requests can make the host rule's list outgrow it (they add one entry
  // each to the <= max_grid / gdy entries of the others), so a chunk size must also leave
  // sum(ceil(max(pages, 1) / chunk)) <= padded.  Both counts fall as the chunk grows, so one bisection serves both, and
  // its result is the host's whenever the host's list fits: always, when no request is empty.
  uint32_t pages_per_chunk = max(max_pages, 1u);
  if (p.split) {
    const uint32_t min_pages = max(128u / (uint32_t)p.req.page_size, 1u);
    pages_per_chunk = smallest_fitting<uint32_t>(min_pages, max_pages, [&](uint32_t n) {
      const uint32_t nb = request_sum(B, red, [&](int b) { return (p.req.pages(b) + n - 1) / n; });
      return (uint64_t)nb * p.gdy > p.max_grid || (uint64_t)nb + empty > (uint64_t)p.padded;
    });
  }

  // exclusive scans of pages (indptr) and of chunks (o_indptr)
  FusedScan<2> scan;
  for (int base = 0; base < B; base += kPlanThreads) {
    const int b = base + tid;
    const bool valid = b < B;
    const int32_t len = valid ? p.req.len(b) : 0;
    const int32_t np = (int32_t)pages_holding(len, p.req.page_size);
    // the host rule counts an empty request as one chunk
    const int32_t nc = !valid ? 0 : p.split ? (int32_t)(((uint32_t)max(np, 1) + pages_per_chunk - 1) / pages_per_chunk) : 1;
    int32_t before[2];
    scan.round({np, nc}, before, wave_tot);
    if (valid) {
      store_page_range(p.csr, b, before[0], len, np, p.req.page_size);
      p.o_indptr[b] = before[1];
    }
  }
  if (tid == 0) {
    p.csr.indptr[B] = scan.carry[0];
    p.o_indptr[B] = scan.carry[1];
    p.chunk_slot[0] = (int32_t)(pages_per_chunk * (uint32_t)p.req.page_size);
    p.chunk_slot[1] = scan.carry[1];
  }
}

// Runs after decode_plan_scan_kernel on the same stream and reads its indptr and o_indptr.
// Every store is bounded by a host-known capacity: the work list by i < padded, a page id by
// indptr[b] + j < sum of pages <= batch * max_blocks.  The list never needs more than padded entries either:
//   unsplit: one entry per request, padded = batch.
//   split:   padded = max(max_grid / gdy, batch), and the search of decode_plan_scan_kernel accepts a chunk size only
//            when its entries, one per empty request included, number <= padded.  One always is accepted: the range's
//            upper end gives one entry per request (batch <= padded, batch * gdy < max_grid), and so does the lower
//            bound an empty range returns.
__global__ __launch_bounds__(kPlanThreads) void decode_plan_fill_kernel(const DevicePlanParams p) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < p.list_blocks) {
    const int i = (int)blockIdx.x * kPlanThreads + tid;
    if (i >= p.padded) return;
    const int32_t total = p.o_indptr[p.req.batch];
    int32_t req = 0, tile = 0;
    if (i < total) {
      req = owner_of(p.o_indptr, p.req.batch, i);  // the request whose chunks hold entry i: every one has >= 1 chunk
      tile = i - p.o_indptr[req];
    }
    p.request_indices[i] = req;
    p.kv_tile_indices[i] = tile;
    if (p.block_valid_mask) p.block_valid_mask[i] = i < total;
    return;
  }
  compact_page_ids(p.req, p.csr, (int)blockIdx.x - p.list_blocks);
}

struct DevicePlanLayout {
  bool split;
  size_t padded;
  uint32_t gdy, max_grid;
  int64_t req_off, tile_off, oind_off, chunk_off, mask_off, indptr_off, indices_off, last_off, v_off, s_off;
  size_t int_bytes, float_bytes;
};

// checks that need no pointer, and the layout of both workspaces: host-known values only
static int device_plan_layout(const fi_batch_decode_plan_device_params_t& a, DevicePlanLayout& l) {
  FI_REQUIRE(a.batch_size > 0 && a.page_size > 0 && a.max_blocks > 0,
             "batch_decode_plan_device: bad batch_size (%d) / page_size (%d) / max_blocks (%d)", a.batch_size,
             a.page_size, a.max_blocks);
  FI_REQUIRE(a.num_kv_heads > 0 && a.num_qo_heads % a.num_kv_heads == 0,
             "batch_decode_plan_device: num_qo_heads (%d) must be a multiple of num_kv_heads (%d)", a.num_qo_heads,
             a.num_kv_heads);
  FI_REQUIRE(a.q_dtype == FI_DTYPE_F16 || a.q_dtype == FI_DTYPE_BF16,
             "batch_decode_plan_device: q dtype must be f16/bf16");
  FI_REQUIRE(decode_kernel_exists(a.kv_dtype, a.head_dim),
             "batch_decode_plan_device: unsupported kv dtype %d / head_dim %d", a.kv_dtype, a.head_dim);
  // 32-bit token and page counts, as the decode kernels hold them
  FI_REQUIRE((int64_t)a.max_blocks * a.page_size < (1ll << 31) && (int64_t)a.batch_size * a.max_blocks < (1ll << 31),
             "batch_decode_plan_device: max_blocks x page_size and batch_size x max_blocks must fit 31 bits");
  const auto [gdy, max_grid] = decode_grid_shape(a.num_qo_heads, a.num_kv_heads, a.head_dim, a.page_size, a.q_dtype,
                                                 a.kv_dtype, a.max_grid_hint);
  l.gdy = gdy;
  l.max_grid = max_grid;
  l.split = (uint64_t)a.batch_size * gdy < max_grid;
  // what the host planner pads a graph plan to when its list is no longer; see decode_plan_fill_kernel for why the
  // list cannot outgrow it
  l.padded = l.split ? std::max((size_t)(max_grid / gdy), (size_t)a.batch_size) : (size_t)a.batch_size;
  const size_t B = (size_t)a.batch_size;
  OffsetAllocator ia(~(size_t)0 >> 1);  // sizes only: the caller's capacity is checked against int_bytes
  l.req_off = ia.alloc(l.padded * sizeof(int32_t));
  l.tile_off = ia.alloc(l.padded * sizeof(int32_t));
  l.oind_off = ia.alloc((B + 1) * sizeof(int32_t));
  l.chunk_off = ia.alloc(2 * sizeof(int32_t));
  l.mask_off = l.split ? ia.alloc(l.padded) : 0;
  l.indptr_off = ia.alloc((B + 1) * sizeof(int32_t));
  l.last_off = ia.alloc(B * sizeof(int32_t));
  l.indices_off = ia.alloc(B * (size_t)a.max_blocks * sizeof(int32_t));
  l.int_bytes = ia.used;
  OffsetAllocator fa(~(size_t)0 >> 1);
  l.v_off = l.s_off = 0;
  if (l.split) {
    l.v_off = fa.alloc((size_t)a.num_qo_heads * l.padded * a.head_dim * sizeof(float));
    l.s_off = fa.alloc((size_t)a.num_qo_heads * l.padded * sizeof(float));
  }
  l.float_bytes = fa.used;
  return 0;
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_batch_decode_plan_device_workspace(const fi_batch_decode_plan_device_params_t* a,
                                                            size_t* int_ws_bytes_out, size_t* float_ws_bytes_out) {
  return plan_workspace_sizes("batch_decode_plan_device_workspace", a, int_ws_bytes_out, float_ws_bytes_out,
                              device_plan_layout);
}

extern "C" FI_API int fi_batch_decode_plan_device(const fi_batch_decode_plan_device_params_t* a,
                                                  int64_t* plan_info_out, int64_t* csr_offsets_out,
                                                  fi_stream_t stream) {
  const char* name = "batch_decode_plan_device";
  FI_REQUIRE(a && plan_info_out && csr_offsets_out, "%s: null argument", name);
  if (check_plan_tensors(name, *a)) return 1;
  DevicePlanLayout l;
  if (device_plan_layout(*a, l)) return 1;
  if (check_plan_workspaces(name, *a, l.int_bytes, l.float_bytes, l.split)) return 1;

  char* ib = (char*)a->int_ws;
  DevicePlanParams p;
  p.req = plan_requests(*a);
  p.request_indices = (int32_t*)(ib + l.req_off);
  p.kv_tile_indices = (int32_t*)(ib + l.tile_off);
  p.o_indptr = (int32_t*)(ib + l.oind_off);
  p.chunk_slot = (int32_t*)(ib + l.chunk_off);
  p.block_valid_mask = l.split ? (uint8_t*)(ib + l.mask_off) : nullptr;
  p.csr = plan_page_table(ib, l.indptr_off, l.indices_off, l.last_off, a->max_blocks);
  p.padded = (int32_t)l.padded;
  p.split = l.split;
  p.gdy = l.gdy;
  p.max_grid = l.max_grid;
  p.list_blocks = (int32_t)ceil_div<size_t>(l.padded, kPlanThreads);
  const int64_t fill_grid = (int64_t)p.list_blocks + (int64_t)a->batch_size * p.csr.row_blocks;
  FI_REQUIRE(l.padded < (1ull << 31) && fill_grid < (1ll << 31), "batch_decode_plan_device: plan too large");

  for (int i = 0; i < FI_DECODE_PLAN_INFO_LEN; ++i) plan_info_out[i] = 0;
  plan_info_out[FI_DP_PADDED_BATCH_SIZE] = (int64_t)l.padded;
  plan_info_out[FI_DP_V_OFFSET] = l.v_off;
  plan_info_out[FI_DP_S_OFFSET] = l.s_off;
  plan_info_out[FI_DP_REQUEST_INDICES_OFFSET] = l.req_off;
  plan_info_out[FI_DP_KV_TILE_INDICES_OFFSET] = l.tile_off;
  plan_info_out[FI_DP_O_INDPTR_OFFSET] = l.oind_off;
  plan_info_out[FI_DP_BLOCK_VALID_MASK_OFFSET] = l.mask_off;
  plan_info_out[FI_DP_KV_CHUNK_SIZE_PTR_OFFSET] = l.chunk_off;
  plan_info_out[FI_DP_ENABLE_CUDA_GRAPH] = 1;
  plan_info_out[FI_DP_SPLIT_KV] = l.split ? 1 : 0;
  plan_info_out[FI_DP_KV_CHUNK_SIZE] = 0;  // on the device only: chunk_slot[0]
  plan_info_out[FI_DP_NUM_WORK] = 0;       // on the device only: chunk_slot[1]
  plan_info_out[FI_DP_BATCH_SIZE] = a->batch_size;
  plan_info_out[FI_DP_INT_BYTES_USED] = (int64_t)l.int_bytes;
  plan_info_out[FI_DP_WINDOW_LEFT] = -1;  // chunks are cut over all pages; a run() with a window masks
  plan_info_out[FI_DP_MAGIC] = FI_DECODE_PLAN_MAGIC;
  plan_info_out[FI_DP_UNIFORM_CHUNKS] = 0;
  csr_offsets_out[0] = l.indptr_off;
  csr_offsets_out[1] = l.indices_off;
  csr_offsets_out[2] = l.last_off;

  return launch_plan_kernels(decode_plan_scan_kernel, decode_plan_fill_kernel, fill_grid, p, stream);
}
