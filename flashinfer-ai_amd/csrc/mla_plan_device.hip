// MLA: the planner that runs on the GPU (fi_batch_mla_plan_device).
//
// It writes what fi_batch_mla_plan(enable_cuda_graph = 1) writes into the int workspace -- the header slots, the merge
// indptr, the MlaItem list in the order request, chunk, row tile -- by the same chunk rule (mla.hip), for
// qo_len = q_len_per_request in every request and kv_len = planned_kv_len(seq_lens, b), from a dense block table and
// lengths that never leave the device.  There is no CSR page table: mla_paged_kernel addresses pages as
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
  const int32_t* seq_lens;
  int32_t* header;        // [4] of kMlaHeaderBytes
  int32_t* merge_indptr;  // [total_rows + 1]
  MlaItem* items;         // [capacity]
  // what the two kernels hand each other
  int32_t* chunk_indptr;  // [batch + 1] scan of chunks per request (>= 1 each)
  int32_t* split_indptr;  // [batch + 1] scan of the chunks of split requests (0 for a request in one chunk)
  int32_t* chunk_slot;    // [1] tokens per chunk
  int64_t block_tables_stride;
  int64_t max_entries;    // partial states the float workspace holds
  int32_t batch, max_blocks, page_size;
  int32_t q_len, num_heads;
  int32_t tiles;          // row tiles per request
  int32_t capacity;       // of the item list
  int32_t items_off;      // header slot kMlaHdrItemsOff
  int32_t split;          // the host-known branch: batch * tiles < max_items
  uint32_t chunk_limit;   // max_items / tiles: the chunks, over all requests, whose items fit max_items
  int32_t list_blocks;    // fill kernel: workgroups that write items; the rest write the merge indptr
};

__device__ __forceinline__ int32_t planned_len(const MlaDevicePlanParams& p, int b) {
  return planned_kv_len(p.seq_lens, b, p.max_blocks, p.page_size);
}
// the host rule counts an empty request as one chunk
__device__ __forceinline__ uint32_t chunks_of(int32_t len, uint32_t chunk) {
  return max(((uint32_t)len + chunk - 1) / chunk, 1u);
}

__global__ __launch_bounds__(kPlanThreads) void mla_plan_scan_kernel(const MlaDevicePlanParams p) {
  __shared__ uint32_t red[kPlanWaves];
  __shared__ int32_t scan_chunks[kPlanWaves], scan_split[kPlanWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int B = p.batch;

  uint32_t max_kv = 0;
  for (int b = tid; b < B; b += kPlanThreads) max_kv = max(max_kv, (uint32_t)planned_len(p, b));
  max_kv = block_reduce<kPlanWaves, RedMax>(max_kv, red);

  // fi_batch_mla_plan's chunk rule (mla.hip), in kMlaTileKV tokens: whole requests when their tiles fill max_items,
  // else smallest_fitting over [kMlaMinChunk / 64, whole / 64].  items = tiles * chunks with the same tiles in every
  // request, so "items > max_items" is "chunks > max_items / tiles" = chunk_limit.  lo, hi and every reduced count are
  // the same in all threads, so the loops are uniform.  A thread's count saturates at chunk_limit + 1 (< 2^22, the
  // host checked), so the sum of kPlanThreads of them fits 32 bits and still compares right.
  const uint32_t whole = max((max_kv + kMlaTileKV - 1) / kMlaTileKV, 1u) * kMlaTileKV;  // < 2^31: the host checked
  uint32_t chunk = whole;
  if (p.split) {
    uint32_t lo = kMlaMinChunk / kMlaTileKV, hi = whole / kMlaTileKV;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) / 2;
      uint64_t n = 0;
      for (int b = tid; b < B; b += kPlanThreads) n += chunks_of(planned_len(p, b), mid * kMlaTileKV);
      uint32_t nc = (uint32_t)min(n, (uint64_t)p.chunk_limit + 1);
      nc = block_reduce<kPlanWaves, RedSum>(nc, red);
      if (nc > p.chunk_limit)
        lo = mid + 1;
      else
        hi = mid;
    }
    chunk = min(whole, lo * kMlaTileKV);  // an empty range leaves its lower bound, as on the host
  }
  // chunks grow until the partial states fit: rows x (chunks of split requests) entries.  chunk < whole only when the
  // search accepted it, so these chunks number <= chunk_limit and their sum needs no saturation.
  const uint64_t rows_per_request = (uint64_t)p.q_len * (uint64_t)p.num_heads;
  while (chunk < whole) {
    uint32_t ns = 0;
    for (int b = tid; b < B; b += kPlanThreads) {
      const uint32_t c = chunks_of(planned_len(p, b), chunk);
      ns += c > 1 ? c : 0;
    }
    ns = block_reduce<kPlanWaves, RedSum>(ns, red);
    if ((uint64_t)ns * rows_per_request <= (uint64_t)p.max_entries) break;
    chunk *= 2;  // < 2 whole < 2^32
  }
  chunk = min(chunk, whole);

  // exclusive scans of chunks and of split chunks, kPlanThreads requests a round
  int32_t carry_chunks = 0, carry_split = 0;
  for (int base = 0; base < B; base += kPlanThreads) {
    const int b = base + tid;
    const bool valid = b < B;
    const int32_t nc = valid ? (int32_t)chunks_of(planned_len(p, b), chunk) : 0;
    const int32_t ns = nc > 1 ? nc : 0;
    // block_incl_scan (common.h) for two values at once, in its barrier convention: two barriers a round
    const int32_t ic = wave_incl_scan(nc), is = wave_incl_scan(ns);
    if (lane == 63) {
      scan_chunks[wave] = ic;
      scan_split[wave] = is;
    }
    __syncthreads();
    int32_t before_chunks = carry_chunks, before_split = carry_split;
#pragma unroll
    for (int w = 0; w < kPlanWaves; ++w) {
      if (w < wave) {
        before_chunks += scan_chunks[w];
        before_split += scan_split[w];
      }
      carry_chunks += scan_chunks[w];
      carry_split += scan_split[w];
    }
    __syncthreads();
    if (valid) {
      p.chunk_indptr[b] = before_chunks + ic - nc;
      p.split_indptr[b] = before_split + is - ns;
    }
  }
  if (tid == 0) {
    p.chunk_indptr[B] = carry_chunks;
    p.split_indptr[B] = carry_split;
    p.chunk_slot[0] = (int32_t)chunk;
    p.header[kMlaHdrMagic] = kMlaWsMagic;
    p.header[kMlaHdrNumWork] = carry_chunks * p.tiles;  // <= capacity, see the file header
    p.header[kMlaHdrItemsOff] = p.items_off;
    p.header[kMlaHdrSplit] = carry_split > 0;
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
    if (i >= p.capacity || i >= p.chunk_indptr[p.batch] * p.tiles) return;
    const int32_t j = i / p.tiles, t = i - j * p.tiles;  // chunk among all requests' chunks, row tile
    // the request that owns chunk j: the last b with chunk_indptr[b] <= j (every request has >= 1 chunk)
    int lo = 0, hi = p.batch - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) / 2;
      if (p.chunk_indptr[mid] <= j)
        lo = mid;
      else
        hi = mid - 1;
    }
    const int b = lo;
    const int32_t first = p.chunk_indptr[b], nc = p.chunk_indptr[b + 1] - first, c = j - first;
    const int32_t len = planned_len(p, b);
    const uint32_t chunk = (uint32_t)p.chunk_slot[0];
    MlaItem it;
    it.qo_start = b * p.q_len;
    it.row0 = t * kMlaRows;
    it.qo_len = p.q_len;
    it.kv_start = (int32_t)((uint32_t)c * chunk);  // < len when c > 0
    it.kv_end = (int32_t)min(((uint32_t)c + 1) * chunk, (uint32_t)len);  // the product < len + chunk < 2^32
    it.kv_len = len;
    it.page_base = (int32_t)((int64_t)b * p.block_tables_stride);
    it.chunk = nc > 1 ? c : -1;
    p.items[i] = it;
    return;
  }
  blk -= p.list_blocks;
  const int64_t row = (int64_t)blk * kPlanThreads + tid;
  const int32_t rows_per_request = p.q_len * p.num_heads;
  const int64_t total_rows = (int64_t)p.batch * rows_per_request;
  if (row > total_rows) return;
  // packed row r of request b starts at the request's first entry + r x its chunks (none for a request in one chunk)
  int32_t entry = p.split_indptr[p.batch] * rows_per_request;
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
  FI_REQUIRE(a && int_ws_bytes_out && float_ws_bytes_out, "batch_mla_plan_device_workspace: null argument");
  MlaDevicePlanLayout l;
  if (mla_device_plan_layout(*a, l)) return 1;
  *int_ws_bytes_out = l.int_bytes;
  *float_ws_bytes_out = 0;  // without room for partial states no request is split
  return 0;
}

extern "C" FI_API int fi_batch_mla_plan_device(const fi_batch_mla_plan_device_params_t* a, int64_t* plan_info_out,
                                               fi_stream_t stream_) {
  FI_REQUIRE(a && plan_info_out, "batch_mla_plan_device: null argument");
  MlaDevicePlanLayout l;
  if (mla_device_plan_layout(*a, l)) return 1;
  FI_REQUIRE(a->block_tables && a->seq_lens && a->int_ws, "batch_mla_plan_device: null tensor");
  FI_REQUIRE(a->block_tables_stride >= a->max_blocks, "batch_mla_plan_device: block table rows overlap");
  // an item's page_base is an int32
  FI_REQUIRE((int64_t)a->batch_size * a->block_tables_stride < (1ll << 31),
             "batch_mla_plan_device: batch_size x block_tables_stride must fit 31 bits");
  FI_REQUIRE(l.int_bytes <= a->int_ws_bytes, "batch_mla_plan_device: int workspace too small (%zu bytes, need %zu)",
             a->int_ws_bytes, l.int_bytes);

  char* ib = (char*)a->int_ws;
  int32_t* scans = (int32_t*)(ib + l.scan_off);
  MlaDevicePlanParams p;
  p.seq_lens = a->seq_lens;
  p.header = (int32_t*)ib;
  p.merge_indptr = (int32_t*)(ib + kMlaHeaderBytes);
  p.items = (MlaItem*)(ib + l.items_off);
  p.chunk_indptr = scans;
  p.split_indptr = scans + a->batch_size + 1;
  p.chunk_slot = scans + 2 * (a->batch_size + 1);
  p.block_tables_stride = a->block_tables_stride;
  // merge indptr entries are int32
  p.max_entries = std::min<int64_t>(mla_max_entries(a->float_ws ? a->float_ws_bytes : 0), (1ll << 31) - 1);
  p.batch = a->batch_size;
  p.max_blocks = a->max_blocks;
  p.page_size = a->page_size;
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

  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(mla_plan_scan_kernel, dim3(1), dim3(kPlanThreads), 0, stream, p);
  FI_HIP_CALL(hipGetLastError());
  hipLaunchKernelGGL(mla_plan_fill_kernel, dim3((uint32_t)fill_grid), dim3(kPlanThreads), 0, stream, p);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}
