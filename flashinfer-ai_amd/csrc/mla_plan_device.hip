// MLA: the planner that runs on the GPU (fi_batch_mla_plan_device).
//
// It writes what fi_batch_mla_plan(enable_cuda_graph = 1) writes into the int workspace -- the header slots, the merge
// indptr, the MlaItem list in the order request, chunk, row tile -- by the same chunk rule (mla.hip), for
// qo_len = q_len_per_request in every request and kv_len = PlanRequests::len(b), the clamped seq_lens[b], from a dense
// block table and lengths that never leave the device.  There is no CSR page table: mla_paged_kernel addresses pages as
// kv_indices[page_base + i], so run() is given kv_indices = block_tables and page_base = b * block_tables_stride, the
// one field that differs from the host plan.
// Two launches, both shaped by host-known values only:
//   mla_plan_scan_kernel   one workgroup: the longest request, the chunk search (one block reduction per round of the
//                          bisection, <= 32 rounds), the doubling while the partial states do not fit (one reduction
//                          per round), the scans of chunks and of split chunks per request, the header
//   mla_plan_fill_kernel   fixed grid: the items from the chunk scan, the merge indptr from the split-chunk scan
// Plain loads and stores; no atomics; nothing is read back.
//
// The list's capacity is host-known, max(max_items, batch * tiles), with tiles = ceil(q_len * H / 16) the same in every
// request:
//   split branch (batch * tiles < max_items): a chunk size the search tested and accepted makes <= max_items items; any
//       other result (the range's upper end untested, the lower bound of an empty range) is min(whole, .) = whole, at
//       least the longest request, so one chunk per request and batch * tiles items;
//   unsplit branch: whole, batch * tiles items;
//   doubling the chunk only merges chunks, so it shrinks either count.
// The partial states fit by the loop's own exit: entries <= mla_max_entries(float_ws_bytes), or chunk = whole and no
// request is split.
#include <algorithm>

#include "mla_plan.h"
#include "plan_device.h"

namespace fi {

struct MlaDevicePlanParams {
  int32_t* header;        // [4] of kMlaHeaderBytes
  int32_t* merge_indptr;  // [total_rows + 1]
  MlaItem* items;         // [capacity]
  // what the two kernels hand each other
  int32_t* chunk_indptr;  // [batch + 1] scan of chunks per request (>= 1 each)
  int32_t* split_indptr;  // [batch + 1] scan of the chunks of split requests (0 for a request in one chunk)
  int32_t* chunk_slot;    // [1] tokens per chunk
  int64_t max_entries;    // partial states the float workspace holds
  PlanRequests req;       // in front of the other scalars (plan_device.h); its block table goes to run(), only the
                          // row stride is read here
  int32_t q_len, num_heads;
  int32_t tiles;          // row tiles per request
  int32_t capacity;       // of the item list
  int32_t items_off;      // header slot kMlaHdrItemsOff
  int32_t split;          // the host-known branch: batch * tiles < max_items
  uint32_t chunk_limit;   // max_items / tiles: the chunks, over all requests, whose items fit max_items
  int32_t list_blocks;    // fill kernel: workgroups that write items; the rest write the merge indptr
};

// the host rule counts an empty request as one chunk
__device__ __forceinline__ uint32_t chunks_of(int32_t len, uint32_t chunk) {
  return max(((uint32_t)len + chunk - 1) / chunk, 1u);
}

__global__ __launch_bounds__(kPlanThreads) void mla_plan_scan_kernel(const MlaDevicePlanParams p) {
  __shared__ uint32_t red[kPlanWaves];
  __shared__ int32_t wave_tot[2][kPlanWaves];
  const int tid = threadIdx.x;
  const int B = p.req.batch;

  uint32_t max_kv = 0;
  for (int b = tid; b < B; b += kPlanThreads) max_kv = max(max_kv, (uint32_t)p.req.len(b));
  max_kv = block_reduce<kPlanWaves, RedMax>(max_kv, red);

  // fi_batch_mla_plan's chunk rule (mla.hip), in kMlaTileKV tokens: whole requests when their tiles fill max_items,
  // else smallest_fitting over [kMlaMinChunk / 64, whole / 64].  items = tiles * chunks with the same tiles in every
  // request, so "items > max_items" is "chunks > max_items / tiles" = chunk_limit.
  const uint32_t whole = max((max_kv + kMlaTileKV - 1) / kMlaTileKV, 1u) * kMlaTileKV;  // < 2^31: the host checked
  uint32_t chunk = whole;
  if (p.split) {
    const uint32_t tiles = smallest_fitting<uint32_t>(kMlaMinChunk / kMlaTileKV, whole / kMlaTileKV, [&](uint32_t n) {
      const auto chunks = [&](int b) { return (uint64_t)chunks_of(p.req.len(b), n * kMlaTileKV); };
      return request_sum<true>(B, red, chunks, p.chunk_limit) > p.chunk_limit;
    });
    chunk = min(whole, tiles * kMlaTileKV);
  }
  // chunks grow until the partial states fit: rows x (chunks of split requests) entries.  chunk < whole only when the
  // search accepted it, so these chunks number <= chunk_limit and their sum needs no saturation.
  const uint64_t rows_per_request = (uint64_t)p.q_len * (uint64_t)p.num_heads;
  while (chunk < whole) {
    const uint32_t ns = request_sum(B, red, [&](int b) {
      const uint32_t c = chunks_of(p.req.len(b), chunk);
      return c > 1 ? c : 0;
    });
    if ((uint64_t)ns * rows_per_request <= (uint64_t)p.max_entries) break;
    chunk *= 2;  // < 2 whole < 2^32
  }
  chunk = min(chunk, whole);

  // exclusive scans of chunks and of split chunks
  FusedScan<2> scan;
  for (int base = 0; base < B; base += kPlanThreads) {
    const int b = base + tid;
    const bool valid = b < B;
    const int32_t nc = valid ? (int32_t)chunks_of(p.req.len(b), chunk) : 0;
    int32_t before[2];
    scan.round({nc, nc > 1 ? nc : 0}, before, wave_tot);
    if (valid) {
      p.chunk_indptr[b] = before[0];
      p.split_indptr[b] = before[1];
    }
  }
  if (tid == 0) {
    p.chunk_indptr[B] = scan.carry[0];
    p.split_indptr[B] = scan.carry[1];
    p.chunk_slot[0] = (int32_t)chunk;
    p.header[kMlaHdrMagic] = kMlaWsMagic;
    p.header[kMlaHdrNumWork] = scan.carry[0] * p.tiles;  // <= capacity, see the file header
    p.header[kMlaHdrItemsOff] = p.items_off;
    p.header[kMlaHdrSplit] = scan.carry[1] > 0;
  }
}

// Runs after mla_plan_scan_kernel on the same stream and reads its two scans and its chunk size.  Every store is
// bounded by a host-known capacity: an item by i < capacity, the merge indptr by row <= total_rows.
__global__ __launch_bounds__(kPlanThreads) void mla_plan_fill_kernel(const MlaDevicePlanParams p) {
  const int tid = threadIdx.x;
  int blk = (int)blockIdx.x;
  if (blk < p.list_blocks) {
    const int i = blk * kPlanThreads + tid;
    // items past the plan's count stay as they were, as the host planner leaves them: the kernel stops at the count
    if (i >= p.capacity || i >= p.chunk_indptr[p.req.batch] * p.tiles) return;
    const int32_t j = i / p.tiles, t = i - j * p.tiles;  // chunk among all requests' chunks, row tile
    const int b = owner_of(p.chunk_indptr, p.req.batch, j);  // every request has >= 1 chunk
    const int32_t first = p.chunk_indptr[b], nc = p.chunk_indptr[b + 1] - first, c = j - first;
    const int32_t len = p.req.len(b);
    const uint32_t chunk = (uint32_t)p.chunk_slot[0];
    MlaItem it;
    it.qo_start = b * p.q_len;
    it.row0 = t * kMlaRows;
    it.qo_len = p.q_len;
    it.kv_start = (int32_t)((uint32_t)c * chunk);  // < len when c > 0
    it.kv_end = (int32_t)min(((uint32_t)c + 1) * chunk, (uint32_t)len);  // the product < len + chunk < 2^32
    it.kv_len = len;
    it.page_base = (int32_t)((int64_t)b * p.req.block_tables_stride);
    it.chunk = nc > 1 ? c : -1;
    p.items[i] = it;
    return;
  }
  blk -= p.list_blocks;
  const int64_t row = (int64_t)blk * kPlanThreads + tid;
  const int32_t rows_per_request = p.q_len * p.num_heads;
  const int64_t total_rows = (int64_t)p.req.batch * rows_per_request;
  if (row > total_rows) return;
  // packed row r of request b starts at the request's first entry + r x its chunks (none for a request in one chunk)
  int32_t entry = p.split_indptr[p.req.batch] * rows_per_request;
  if (row < total_rows) {
    const int b = (int)(row / rows_per_request), r = (int)(row - (int64_t)b * rows_per_request);
    const int32_t first = p.split_indptr[b];
    entry = first * rows_per_request + r * (p.split_indptr[b + 1] - first);
  }
  p.merge_indptr[row] = entry;
}

struct MlaDevicePlanLayout {
  bool split;
  int64_t max_items, tiles, total_rows, capacity;
  int64_t items_off, scan_off;  // bytes; the scans: chunk_indptr [batch + 1], split_indptr [batch + 1], chunk size [1]
  size_t int_bytes;
  size_t float_bytes = 0;  // the least: without room for partial states no request is split
};

// checks that need no pointer, and the layout of the int workspace: host-known values only
static int mla_device_plan_layout(const fi_batch_mla_plan_device_params_t& a, MlaDevicePlanLayout& l) {
  FI_REQUIRE(a.head_dim_ckv == kMlaCkv, "batch_mla_plan_device: unsupported head_dim_ckv %d (only 512)",
             a.head_dim_ckv);
  FI_REQUIRE(a.head_dim_kpe == kMlaKpe, "batch_mla_plan_device: unsupported head_dim_kpe %d (only 64)",
             a.head_dim_kpe);
  FI_REQUIRE(a.q_dtype == a.kv_dtype, "batch_mla_plan_device: q dtype %d and kv dtype %d differ (dtype mismatch)",
             a.q_dtype, a.kv_dtype);
  FI_REQUIRE(a.q_dtype == FI_DTYPE_F16 || a.q_dtype == FI_DTYPE_BF16,
             "batch_mla_plan_device: unsupported dtype %d (f16 / bf16)", a.q_dtype);
  FI_REQUIRE(a.batch_size > 0 && a.page_size > 0 && a.max_blocks > 0 && a.num_heads > 0 && a.q_len_per_request > 0,
             "batch_mla_plan_device: bad batch_size (%d) / page_size (%d) / max_blocks (%d) / num_heads (%d) / "
             "q_len_per_request (%d)",
             a.batch_size, a.page_size, a.max_blocks, a.num_heads, a.q_len_per_request);
  // 32-bit tokens, with room to round the longest request up to a tile, and 32-bit packed rows, as the kernel holds
  // them
  FI_REQUIRE((int64_t)a.max_blocks * a.page_size < (1ll << 31) - kMlaTileKV,
             "batch_mla_plan_device: max_blocks x page_size must fit 31 bits");
  const int64_t rows_per_request = (int64_t)a.q_len_per_request * a.num_heads;
  l.total_rows = a.batch_size * rows_per_request;
  FI_REQUIRE(l.total_rows < (1ll << 31) - kMlaRows, "batch_mla_plan_device: too many rows");
  l.max_items = a.max_items_hint > 0 ? a.max_items_hint
                                     : std::max<int64_t>(kMlaWgPerCu * (int64_t)fi_num_compute_units(), 1);
  FI_REQUIRE(l.max_items < (1 << 22), "batch_mla_plan_device: max_items_hint %lld too large", (long long)l.max_items);
  l.tiles = ceil_div<int64_t>(rows_per_request, kMlaRows);
  const int64_t total_tiles = a.batch_size * l.tiles;
  l.split = total_tiles < l.max_items;
  // see the file header for why the list cannot outgrow this
  l.capacity = std::max(l.max_items, total_tiles);
  FI_REQUIRE(l.capacity < (1ll << 31), "batch_mla_plan_device: too many work items");
  l.items_off = mla_items_offset(l.total_rows);
  l.scan_off = l.items_off + l.capacity * (int64_t)sizeof(MlaItem);
  l.int_bytes = (size_t)(l.scan_off + (2 * ((int64_t)a.batch_size + 1) + 1) * 4);
  FI_REQUIRE(l.items_off < (1ll << 31), "batch_mla_plan_device: too many rows");
  return 0;
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_batch_mla_plan_device_workspace(const fi_batch_mla_plan_device_params_t* a,
                                                         size_t* int_ws_bytes_out, size_t* float_ws_bytes_out) {
  return plan_workspace_sizes("batch_mla_plan_device_workspace", a, int_ws_bytes_out, float_ws_bytes_out,
                              mla_device_plan_layout);
}

extern "C" FI_API int fi_batch_mla_plan_device(const fi_batch_mla_plan_device_params_t* a, int64_t* plan_info_out,
                                               fi_stream_t stream) {
  const char* name = "batch_mla_plan_device";
  FI_REQUIRE(a && plan_info_out, "%s: null argument", name);
  MlaDevicePlanLayout l;
  if (mla_device_plan_layout(*a, l)) return 1;
  if (check_plan_tensors(name, *a)) return 1;
  // an item's page_base is an int32
  FI_REQUIRE((int64_t)a->batch_size * a->block_tables_stride < (1ll << 31),
             "batch_mla_plan_device: batch_size x block_tables_stride must fit 31 bits");
  if (check_plan_workspaces(name, *a, l.int_bytes, l.float_bytes, /*split=*/false)) return 1;

  char* ib = (char*)a->int_ws;
  int32_t* scans = (int32_t*)(ib + l.scan_off);
  MlaDevicePlanParams p;
  p.req = plan_requests(*a);
  p.header = (int32_t*)ib;
  p.merge_indptr = (int32_t*)(ib + kMlaHeaderBytes);
  p.items = (MlaItem*)(ib + l.items_off);
  p.chunk_indptr = scans;
  p.split_indptr = scans + a->batch_size + 1;
  p.chunk_slot = scans + 2 * (a->batch_size + 1);
  // merge indptr entries are int32
  p.max_entries = std::min<int64_t>(mla_max_entries(a->float_ws ? a->float_ws_bytes : 0), (1ll << 31) - 1);
  p.q_len = a->q_len_per_request;
  p.num_heads = a->num_heads;
  p.tiles = (int32_t)l.tiles;
  p.capacity = (int32_t)l.capacity;
  p.items_off = (int32_t)l.items_off;
  p.split = l.split;
  p.chunk_limit = (uint32_t)(l.max_items / l.tiles);
  p.list_blocks = (int32_t)ceil_div<int64_t>(l.capacity, kPlanThreads);
  const int64_t fill_grid = p.list_blocks + ceil_div<int64_t>(l.total_rows + 1, kPlanThreads);

  for (int i = 0; i < FI_MLA_PLAN_INFO_LEN; ++i) plan_info_out[i] = 0;
  plan_info_out[FI_MLA_NUM_WORK] = 0;  // decided on the device: header slot kMlaHdrNumWork
  plan_info_out[FI_MLA_GRID] = l.max_items;
  plan_info_out[FI_MLA_TOTAL_ROWS] = l.total_rows;
  plan_info_out[FI_MLA_KV_CHUNK_SIZE] = 0;  // decided on the device: in the items only
  plan_info_out[FI_MLA_SPLIT_KV] = 0;       // decided on the device: header slot kMlaHdrSplit; run() merges anyway
  plan_info_out[FI_MLA_ENABLE_CUDA_GRAPH] = 1;
  plan_info_out[FI_MLA_NUM_HEADS] = a->num_heads;
  plan_info_out[FI_MLA_BATCH_SIZE] = a->batch_size;
  plan_info_out[FI_MLA_INT_BYTES_USED] = (int64_t)l.int_bytes;
  plan_info_out[FI_MLA_MERGE_INDPTR_OFFSET] = kMlaHeaderBytes;
  plan_info_out[FI_MLA_ITEMS_OFFSET] = l.items_off;
  plan_info_out[FI_MLA_NUM_ENTRIES] = 0;  // decided on the device: merge_indptr[total_rows] <= what float_ws holds
  plan_info_out[FI_MLA_V_OFFSET] = mla_v_offset(a->float_ws_bytes);
  plan_info_out[FI_MLA_PAGE_SIZE] = a->page_size;
  plan_info_out[FI_MLA_DTYPE] = a->q_dtype;
  plan_info_out[FI_MLA_MAGIC] = FI_MLA_PLAN_MAGIC;

  return launch_plan_kernels(mla_plan_scan_kernel, mla_plan_fill_kernel, fill_grid, p, stream);
}
