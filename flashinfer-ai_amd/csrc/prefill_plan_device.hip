// Batch prefill: the planner that runs on the GPU (fi_batch_prefill_plan_device).
//
// It writes what fi_batch_prefill_plan(enable_cuda_graph = 1, causal = 1) writes -- the work list with its -1 padding,
// merge_indptr, the kv-chunk-size slot -- by the same rule (measure_batch, kv_span, choose_kv_chunk with graph_items
// != 0, prefill.hip), plus the CSR page table and the qo_indptr the prefill kernels read, from a dense block table,
// lengths and query offsets that never leave the device.  The list is in request order: the host's sort by cost and
// its interleave of wide and narrow items are not done here.
// Two launches, both shaped by host-known values only:
//   prefill_plan_scan_kernel   one workgroup: the clamped qo_indptr, the longest span, the chunk search (one block
//                              reduction per round of the bisection, <= 32 rounds), the scans for the page indptr,
//                              the items and the partial-state entries per request
//   prefill_plan_fill_kernel   fixed grid: the work list from the item scan, merge_indptr from the entry scan, the
//                              page ids compacted by indptr
// Plain vector loads and stores; no atomics; nothing is read back.
#include <algorithm>

#include "plan_device.h"
#include "prefill_plan.h"

namespace fi {

struct PrefillDevicePlanParams {
  // work list (fi_prefill_plan_slot offsets of the int workspace)
  int32_t* request_indices;  // [capacity]
  int32_t* qo_tile_indices;  // [capacity]
  int32_t* kv_tile_indices;  // [capacity]
  int32_t* merge_indptr;     // [total_num_rows + 1]
  int32_t* chunk_slot;       // [2]: tokens per chunk, real work items
  const int32_t* cum_seq_lens_q;  // [batch + 1] the caller's; beside the copy that is made from it
  // what the two kernels hand each other, and the kernels of run() read
  int32_t* qo_indptr;     // [batch + 1] first query row per request: cum_seq_lens_q clamped, non-decreasing
  int32_t* item_indptr;   // [batch + 1] scan of q tiles x chunks
  int32_t* entry_indptr;  // [batch + 1] scan of query rows x chunks
  PlanPageTable csr;
  PlanRequests req;  // in front of the other scalars (plan_device.h)
  int32_t total_num_rows, group, window_left;
  int32_t capacity;    // of the work list
  int32_t split;       // the host-known branch: ceil(total_num_rows * group / 128) <= max_items
  uint32_t max_items;  // items a chunk size may make
  // fill kernel: workgroups that write the work list, then merge_indptr; the rest compact page ids
  int32_t list_blocks, merge_blocks;
};

// keys the chunks of request b are cut from: kv_span of the host rule under the causal mask
__device__ __forceinline__ uint32_t span_of(const PrefillDevicePlanParams& p, int b) {
  return (uint32_t)kv_span(p.req.len(b), 0, /*causal=*/true, p.window_left);
}
__device__ __forceinline__ int32_t rows_of(const PrefillDevicePlanParams& p, int b) {
  return p.qo_indptr[b + 1] - p.qo_indptr[b];
}
// 128-row q tiles over rows x group packed rows (total_num_rows x group fits 31 bits: the host checked)
__device__ __forceinline__ uint32_t q_tiles_of(const PrefillDevicePlanParams& p, int32_t rows) {
  return ((uint32_t)rows * (uint32_t)p.group + kPlanTileQ - 1) / kPlanTileQ;
}
__device__ __forceinline__ uint32_t chunks_of(uint32_t span, uint32_t chunk) { return (span + chunk - 1) / chunk; }

__global__ __launch_bounds__(kPlanThreads) void prefill_plan_scan_kernel(const PrefillDevicePlanParams p) {
  __shared__ uint32_t red[kPlanWaves];
  __shared__ int32_t wave_tot[3][kPlanWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int B = p.req.batch;

  // qo_indptr[b] = max over j <= b of clamp(cum_seq_lens_q[j], 0, total_num_rows): an inclusive scan with max in the
  // place of wave_incl_scan's sum, kPlanThreads entries a round.  Whatever the caller's tensor holds, the requests'
  // row ranges are then disjoint, in order and inside the output.
  int32_t row_carry = 0;
  for (int base = 0; base <= B; base += kPlanThreads) {
    const int b = base + tid;
    int32_t v = b <= B ? min(max(p.cum_seq_lens_q[b], 0), p.total_num_rows) : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t o = __shfl_up(v, d, 64);
      if (lane >= d) v = max(v, o);
    }
    if (lane == 63) wave_tot[0][wave] = v;
    __syncthreads();
    int32_t before = row_carry;
#pragma unroll
    for (int w = 0; w < kPlanWaves; ++w) {
      if (w < wave) before = max(before, wave_tot[0][w]);
      row_carry = max(row_carry, wave_tot[0][w]);
    }
    __syncthreads();
    if (b <= B) p.qo_indptr[b] = max(before, v);
  }
  __syncthreads();  // rows_of() below reads entries other threads of this workgroup stored

  uint32_t max_span = 1;
  for (int b = tid; b < B; b += kPlanThreads) max_span = max(max_span, span_of(p, b));
  max_span = block_reduce<kPlanWaves, RedMax>(max_span, red);

  // choose_kv_chunk with graph_items != 0 (prefill.hip): smallest_fitting over [2, ceil(max_span / 64)] kv tiles, the
  // items counted against max_items; no price model, no balance rule.  In the unsplit branch the host knows that
  // nothing fits, and the result is the range's upper end, one chunk per request.
  const uint32_t hi_tiles = (max_span + kPlanTileKV - 1) / kPlanTileKV;
  uint32_t chunk_tiles = max(hi_tiles, 2u);
  if (p.split)
    chunk_tiles = smallest_fitting<uint32_t>(2, hi_tiles, [&](uint32_t n) {
      const auto items = [&](int b) {
        return (uint64_t)q_tiles_of(p, rows_of(p, b)) * chunks_of(span_of(p, b), n * kPlanTileKV);
      };
      return request_sum<true>(B, red, items, p.max_items) > p.max_items;
    });
  const uint32_t chunk = chunk_tiles * kPlanTileKV;

  // exclusive scans of pages (indptr), of items and of partial-state entries
  FusedScan<3> scan;
  for (int base = 0; base < B; base += kPlanThreads) {
    const int b = base + tid;
    const bool valid = b < B;
    const int32_t len = valid ? p.req.len(b) : 0;
    const int32_t np = (int32_t)pages_holding(len, p.req.page_size);
    const int32_t rows = valid ? rows_of(p, b) : 0;
    const int32_t nc = valid ? (int32_t)chunks_of(span_of(p, b), chunk) : 0;
    int32_t before[3];
    scan.round({np, (int32_t)q_tiles_of(p, rows) * nc, rows * nc}, before, wave_tot);
    if (valid) {
      store_page_range(p.csr, b, before[0], len, np, p.req.page_size);
      p.item_indptr[b] = before[1];
      p.entry_indptr[b] = before[2];
    }
  }
  if (tid == 0) {
    p.csr.indptr[B] = scan.carry[0];
    p.item_indptr[B] = scan.carry[1];
    p.entry_indptr[B] = scan.carry[2];
    p.chunk_slot[0] = (int32_t)chunk;
    p.chunk_slot[1] = scan.carry[1];
  }
}

// Runs after prefill_plan_scan_kernel on the same stream and reads its scans and its chunk slot.
// Every store is bounded by a host-known capacity: the work list by i < capacity, merge_indptr by
// row <= total_num_rows, a page id by indptr[b] + j < sum of pages <= batch * max_blocks.  Nothing needs more either.
// With R = total_num_rows, G = group, T0 = ceil(R G / 128), and the clamped qo_indptr giving sum(rows_b) <= R:
//   q tiles     sum(ceil(rows_b G / 128)) <= T0 + batch - 1 (every request rounds up by less than one tile).
//   work list   a chunk size the search accepted makes <= max_items items; any other result of the search (the range's
//               upper end untested, the lower bound of an empty range, the unsplit branch) is >= the longest span, so
//               one chunk per request and one item per q tile.  capacity = max(max_items, T0 + batch - 1) when split,
//               T0 + batch - 1 when not, covers both.
//   entries     (query row, chunk) pairs, the partial states a split run() writes.  Each pair lies in an item, and an
//               item's 128 packed rows touch <= rpi = ceil(128 / G) + 1 query rows, so an accepted chunk size makes
//               <= max_items x rpi of them.  One chunk per request makes sum(rows_b) <= R of them, and the split branch
//               has T0 <= max_items, so R <= 128 max_items / G <= max_items x ceil(128 / G).  E_max = max_items x rpi
//               bounds both, and the float workspace is sized for it.
__global__ __launch_bounds__(kPlanThreads) void prefill_plan_fill_kernel(const PrefillDevicePlanParams p) {
  const int tid = threadIdx.x;
  const uint32_t chunk = (uint32_t)p.chunk_slot[0];
  int blk = (int)blockIdx.x;
  if (blk < p.list_blocks) {
    const int i = blk * kPlanThreads + tid;
    if (i >= p.capacity) return;
    int32_t req = -1, tile = 0, kvt = 0;  // -1: a padding item, as the host pads; the workgroup exits
    if (i < p.item_indptr[p.req.batch]) {
      req = owner_of(p.item_indptr, p.req.batch, i);
      const int32_t nc = (int32_t)chunks_of(span_of(p, req), chunk);  // >= 1
      const int32_t first = p.item_indptr[req];
      const int32_t q_tiles = (p.item_indptr[req + 1] - first) / nc;
      const int32_t t = (i - first) / nc;
      kvt = (i - first) - t * nc;
      tile = q_tiles - 1 - t;  // under the causal mask the later q tiles are the heavier: they go first
    }
    p.request_indices[i] = req;
    p.qo_tile_indices[i] = tile;
    p.kv_tile_indices[i] = kvt;
    return;
  }
  blk -= p.list_blocks;
  if (blk < p.merge_blocks) {
    const int row = blk * kPlanThreads + tid;
    if (row > p.total_num_rows) return;
    // rows no request owns (before qo_indptr[0], from qo_indptr[batch] on) get empty ranges: the merge skips them
    int32_t entry = 0;
    if (row >= p.qo_indptr[p.req.batch]) {
      entry = p.entry_indptr[p.req.batch];
    } else if (row >= p.qo_indptr[0]) {
      const int b = owner_of(p.qo_indptr, p.req.batch, row);
      entry = p.entry_indptr[b] + (row - p.qo_indptr[b]) * (int32_t)chunks_of(span_of(p, b), chunk);
    }
    p.merge_indptr[row] = entry;
    return;
  }
  compact_page_ids(p.req, p.csr, blk - p.merge_blocks);
}

struct PrefillDevicePlanLayout {
  bool split;
  size_t capacity;
  int64_t max_items;
  int64_t req_off, tile_off, kvt_off, mrg_off, chunk_off, qo_off, item_off, entry_off, indptr_off, indices_off,
      last_off, v_off, s_off;
  size_t int_bytes, float_bytes;
};

// checks that need no pointer, and the layout of both workspaces: host-known values only
static int prefill_device_plan_layout(const fi_batch_prefill_plan_device_params_t& a, PrefillDevicePlanLayout& l) {
  FI_REQUIRE(a.batch_size > 0 && a.page_size > 0 && a.max_blocks > 0 && a.total_num_rows >= 0,
             "batch_prefill_plan_device: bad batch_size (%d) / page_size (%d) / max_blocks (%d) / total_num_rows (%d)",
             a.batch_size, a.page_size, a.max_blocks, a.total_num_rows);
  FI_REQUIRE(a.num_kv_heads > 0 && a.num_qo_heads > 0 && a.num_qo_heads % a.num_kv_heads == 0,
             "batch_prefill_plan_device: num_qo_heads (%d) must be a multiple of num_kv_heads (%d)", a.num_qo_heads,
             a.num_kv_heads);
  const bool q16 = a.q_dtype == FI_DTYPE_F16 || a.q_dtype == FI_DTYPE_BF16;
  FI_REQUIRE(q16 || a.q_dtype == FI_DTYPE_FP8_E4M3, "batch_prefill_plan_device: q dtype must be f16 / bf16 / fp8 e4m3");
  FI_REQUIRE(a.kv_dtype == a.q_dtype || (q16 && (a.kv_dtype == FI_DTYPE_FP8_E4M3 || a.kv_dtype == FI_DTYPE_FP8_E5M2)),
             "batch_prefill_plan_device: unsupported kv dtype %d under q dtype %d (the q dtype, or fp8 under f16 / bf16)",
             a.kv_dtype, a.q_dtype);
  FI_REQUIRE(a.head_dim == 64 || a.head_dim == 128 || a.head_dim == 256,
             "batch_prefill_plan_device: unsupported head_dim %d (64/128/256)", a.head_dim);
  const int64_t group = a.num_qo_heads / a.num_kv_heads;
  // 32-bit token, page and packed-row counts, as the prefill kernels hold them; room to round a span up to a chunk
  FI_REQUIRE((int64_t)a.max_blocks * a.page_size < (1ll << 31) - 4 * kPlanTileKV &&
                 (int64_t)a.batch_size * a.max_blocks < (1ll << 31) &&
                 (int64_t)a.total_num_rows * group < (1ll << 31) - kPlanTileQ,
             "batch_prefill_plan_device: max_blocks x page_size, batch_size x max_blocks and total_num_rows x group "
             "must fit 31 bits");
  l.max_items = a.max_items_hint > 0 ? a.max_items_hint : resident_items(a.num_kv_heads);
  FI_REQUIRE(l.max_items < (1 << 22), "batch_prefill_plan_device: max_items_hint %lld too large",
             (long long)l.max_items);
  const int64_t q_tiles = ceil_div<int64_t>((int64_t)a.total_num_rows * group, kPlanTileQ);
  const size_t B = (size_t)a.batch_size, bound = (size_t)q_tiles + B - 1;
  l.split = q_tiles <= l.max_items;
  // see prefill_plan_fill_kernel for why neither the list nor the partial states can outgrow these
  l.capacity = l.split ? std::max((size_t)l.max_items, bound) : bound;
  OffsetAllocator ia(~(size_t)0 >> 1);  // sizes only: the caller's capacity is checked against int_bytes
  l.req_off = ia.alloc(l.capacity * sizeof(int32_t));
  l.tile_off = ia.alloc(l.capacity * sizeof(int32_t));
  l.kvt_off = ia.alloc(l.capacity * sizeof(int32_t));
  l.mrg_off = ia.alloc(((size_t)a.total_num_rows + 1) * sizeof(int32_t));
  l.chunk_off = ia.alloc(2 * sizeof(int32_t));
  l.qo_off = ia.alloc((B + 1) * sizeof(int32_t));
  l.item_off = ia.alloc((B + 1) * sizeof(int32_t));
  l.entry_off = ia.alloc((B + 1) * sizeof(int32_t));
  l.indptr_off = ia.alloc((B + 1) * sizeof(int32_t));
  l.last_off = ia.alloc(B * sizeof(int32_t));
  l.indices_off = ia.alloc(B * (size_t)a.max_blocks * sizeof(int32_t));
  l.int_bytes = ia.used;
  OffsetAllocator fa(~(size_t)0 >> 1);
  l.v_off = l.s_off = 0;
  if (l.split) {
    // lse first, then the outputs, as fi_batch_prefill_plan lays a graph plan out
    const size_t entries = (size_t)l.max_items * (size_t)(ceil_div<int64_t>(kPlanTileQ, group) + 1);
    l.s_off = fa.alloc(entries * a.num_qo_heads * sizeof(float));
    l.v_off = fa.alloc(entries * a.num_qo_heads * a.head_dim * sizeof(float));
  }
  l.float_bytes = fa.used;
  return 0;
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_batch_prefill_plan_device_workspace(const fi_batch_prefill_plan_device_params_t* a,
                                                             size_t* int_ws_bytes_out, size_t* float_ws_bytes_out) {
  return plan_workspace_sizes("batch_prefill_plan_device_workspace", a, int_ws_bytes_out, float_ws_bytes_out,
                              prefill_device_plan_layout);
}

extern "C" FI_API int fi_batch_prefill_plan_device(const fi_batch_prefill_plan_device_params_t* a,
                                                   int64_t* plan_info_out, int64_t* csr_offsets_out,
                                                   fi_stream_t stream) {
  const char* name = "batch_prefill_plan_device";
  FI_REQUIRE(a && plan_info_out && csr_offsets_out, "%s: null argument", name);
  if (check_plan_tensors(name, *a, a->cum_seq_lens_q != nullptr)) return 1;
  PrefillDevicePlanLayout l;
  if (prefill_device_plan_layout(*a, l)) return 1;
  if (check_plan_workspaces(name, *a, l.int_bytes, l.float_bytes, l.split)) return 1;

  char* ib = (char*)a->int_ws;
  auto at = [&](int64_t off) { return (int32_t*)(ib + off); };
  PrefillDevicePlanParams p;
  p.req = plan_requests(*a);
  p.cum_seq_lens_q = a->cum_seq_lens_q;
  p.request_indices = at(l.req_off);
  p.qo_tile_indices = at(l.tile_off);
  p.kv_tile_indices = at(l.kvt_off);
  p.merge_indptr = at(l.mrg_off);
  p.chunk_slot = at(l.chunk_off);
  p.qo_indptr = at(l.qo_off);
  p.item_indptr = at(l.item_off);
  p.entry_indptr = at(l.entry_off);
  p.csr = plan_page_table(ib, l.indptr_off, l.indices_off, l.last_off, a->max_blocks);
  p.total_num_rows = a->total_num_rows;
  p.group = a->num_qo_heads / a->num_kv_heads;
  p.window_left = a->window_left < 0 ? -1 : a->window_left;
  p.capacity = (int32_t)l.capacity;
  p.split = l.split;
  p.max_items = (uint32_t)l.max_items;
  p.list_blocks = (int32_t)ceil_div<size_t>(l.capacity, kPlanThreads);
  p.merge_blocks = (int32_t)ceil_div<size_t>((size_t)a->total_num_rows + 1, kPlanThreads);
  const int64_t fill_grid = (int64_t)p.list_blocks + p.merge_blocks + (int64_t)a->batch_size * p.csr.row_blocks;
  FI_REQUIRE(l.capacity < (1ull << 31) && fill_grid < (1ll << 31), "batch_prefill_plan_device: plan too large");

  for (int i = 0; i < FI_PREFILL_PLAN_INFO_LEN; ++i) plan_info_out[i] = 0;
  plan_info_out[FI_PP_PADDED_BATCH_SIZE] = (int64_t)l.capacity;
  plan_info_out[FI_PP_TOTAL_NUM_ROWS] = a->total_num_rows;
  plan_info_out[FI_PP_KV_CHUNK_SIZE_PTR_OFFSET] = l.chunk_off;
  plan_info_out[FI_PP_CTA_TILE_Q] = kPlanTileQ;
  plan_info_out[FI_PP_REQUEST_INDICES_OFFSET] = l.req_off;
  plan_info_out[FI_PP_QO_TILE_INDICES_OFFSET] = l.tile_off;
  plan_info_out[FI_PP_KV_TILE_INDICES_OFFSET] = l.kvt_off;
  plan_info_out[FI_PP_MERGE_INDPTR_OFFSET] = l.mrg_off;
  plan_info_out[FI_PP_BATCH_SIZE] = a->batch_size;
  plan_info_out[FI_PP_KV_CHUNK_SIZE] = 0;  // on the device only: chunk_slot[0]
  plan_info_out[FI_PP_V_OFFSET] = l.v_off;
  plan_info_out[FI_PP_S_OFFSET] = l.s_off;
  plan_info_out[FI_PP_NUM_WORK] = 0;  // on the device only: chunk_slot[1]
  plan_info_out[FI_PP_ENABLE_CUDA_GRAPH] = 1;
  plan_info_out[FI_PP_SPLIT_KV] = l.split ? 1 : 0;
  plan_info_out[FI_PP_MAGIC] = FI_PREFILL_PLAN_MAGIC;
  csr_offsets_out[0] = l.indptr_off;
  csr_offsets_out[1] = l.indices_off;
  csr_offsets_out[2] = l.last_off;
  csr_offsets_out[3] = l.qo_off;

  return launch_plan_kernels(prefill_plan_scan_kernel, prefill_plan_fill_kernel, fill_grid, p, stream);
}
