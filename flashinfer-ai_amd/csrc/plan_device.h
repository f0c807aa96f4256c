// What the planners that run on the GPU (decode_plan_device.hip, prefill_plan_device.hip, mla_plan_device.hip) share.
// Each is two launches: a scan kernel of ONE workgroup of kPlanThreads threads that loops over the requests, and a fill
// kernel on a fixed grid.  Here are the requests as they read them (the length clamp), the per-request sum and the rule
// for the chunk search, the fused scan round, the owner search of the fill kernels, the CSR page table that two of
// them cut from the block table, and the host side of an entry: argument checks, workspace sizes, the launch pair.
#pragma once
#include <type_traits>

#include "common.h"

namespace fi {

constexpr int kPlanThreads = 256;
constexpr int kPlanWaves = kPlanThreads / 64;

__device__ __forceinline__ uint32_t pages_holding(int32_t len, int32_t page_size) {
  return ((uint32_t)len + (uint32_t)page_size - 1) / (uint32_t)page_size;
}
// tokens in the last of the np pages that hold len tokens; 0 for a request without a page
__device__ __forceinline__ int32_t last_page_tokens(int32_t len, int32_t np, int32_t page_size) {
  return np > 0 ? len - (np - 1) * page_size : 0;
}

// The requests of a plan-free call: a dense block table and lengths that never leave the device.
struct PlanRequests {
  const int32_t* block_tables;  // [batch, max_blocks], rows block_tables_stride apart
  const int32_t* seq_lens;      // [batch]
  int64_t block_tables_stride;
  int32_t batch, max_blocks, page_size;
  int32_t row_tokens;  // max_blocks * page_size, what a block-table row can hold: below 2^31, every entry checks
  // tokens of request b the plan covers: the length clamped to what its row can hold (a negative one: 0)
  __device__ __forceinline__ int32_t len(int b) const { return min(max(seq_lens[b], 0), row_tokens); }
  __device__ __forceinline__ uint32_t pages(int b) const { return pages_holding(len(b), page_size); }
};
// A params struct holds its PlanRequests right in front of its own scalars.  The struct has no padding, so those
// follow batch .. row_tokens without a gap and a scan kernel fetches them all with one load at its top, as when they
// were loose fields; with a gap the second load waits where it is first used, 0.1-0.2 us of a planner's ~13 (3.14).
static_assert(sizeof(PlanRequests) == 3 * 8 + 4 * 4, "PlanRequests has no padding");
template <class Args>
PlanRequests plan_requests(const Args& a) {
  return {a.block_tables, a.seq_lens, a.block_tables_stride, a.batch_size, a.max_blocks, a.page_size,
          a.max_blocks * a.page_size};
}

// ---- the chunk search ----
// The device planners call smallest_fitting (common.h), the function the host planners call, with 32-bit bounds.  Its
// predicate holds a block reduction (request_sum below), so EVERY thread of the workgroup makes the call, with the
// same lo and hi; the reduced count is the same in all threads, which keeps the bisection uniform.

// The sum of count(b) over the requests, in every thread: one strided pass and a block reduction over `red`
// (kPlanWaves words).  Every thread of the workgroup makes the call.  With SATURATE a thread's share is summed in 64
// bits and cut at limit + 1 (limit < 2^22: the host checked), so the sum of kPlanThreads shares fits 32 bits and
// still compares right with limit.
template <bool SATURATE = false, class Count>
__device__ __forceinline__ uint32_t request_sum(int batch, uint32_t* red, Count count, uint32_t limit = 0) {
  std::conditional_t<SATURATE, uint64_t, uint32_t> n = 0;
  for (int b = threadIdx.x; b < batch; b += kPlanThreads) n += count(b);
  if constexpr (SATURATE) n = min(n, (uint64_t)limit + 1);
  return block_reduce<kPlanWaves, RedSum>((uint32_t)n, red);
}

// ---- the fused scan round ----
// Exclusive prefix sums of N values per request, kPlanThreads requests a round, the carries of the rounds before
// included.  It is block_incl_scan (common.h) for N values at once, in its barrier convention: N wave scans, N words
// per wave published, barrier, the waves in front summed and the carries advanced, barrier -- two barriers a round
// whatever N is.  As N block_incl_scan calls, 2 N barriers, the decode planner's two launches measured 0.2-0.5 us of
// 9.5 slower, so the planners scan through this and not through N calls.
// Every thread of the workgroup makes each call, in uniform control flow; a thread past the batch passes zeros.
// `wave_tot` is N x kPlanWaves words of LDS that nobody reads between the calls.
template <int N>
struct FusedScan {
  int32_t carry[N] = {};  // the sums over the rounds so far: the totals, after the last round
  __device__ __forceinline__ void round(const int32_t (&v)[N], int32_t (&before)[N],
                                        int32_t (*wave_tot)[kPlanWaves]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t incl[N];
#pragma unroll
    for (int i = 0; i < N; ++i) incl[i] = wave_incl_scan(v[i]);
    if (lane == 63) {
#pragma unroll
      for (int i = 0; i < N; ++i) wave_tot[i][wave] = incl[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) before[i] = carry[i];
#pragma unroll
    for (int w = 0; w < kPlanWaves; ++w) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        if (w < wave) before[i] += wave_tot[i][w];
        carry[i] += wave_tot[i][w];
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) before[i] += incl[i] - v[i];
  }
};

// the last b in [0, batch) with indptr[b] <= x, for a non-decreasing indptr with indptr[0] <= x: the request that owns
// item or row x when x < indptr[batch] (requests that own nothing repeat their neighbour's value and are passed over)
__device__ __forceinline__ int owner_of(const int32_t* indptr, int batch, int32_t x) {
  int lo = 0, hi = batch - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (indptr[mid] <= x)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// ---- the CSR page table the decode and prefill kernels address the cache through ----
struct PlanPageTable {
  int32_t* indptr;         // [batch + 1]
  int32_t* indices;        // [batch * max_blocks]
  int32_t* last_page_len;  // [batch]
  int32_t row_blocks;      // fill kernel: workgroups per block-table row
};
inline PlanPageTable plan_page_table(void* int_ws, int64_t indptr_off, int64_t indices_off, int64_t last_off,
                                     int32_t max_blocks) {
  char* ib = (char*)int_ws;
  return {(int32_t*)(ib + indptr_off), (int32_t*)(ib + indices_off), (int32_t*)(ib + last_off),
          ceil_div(max_blocks, kPlanThreads)};
}
// scan kernel, request b of a round: its np pages start at pages_before, the exclusive scan of the page counts
// (the thread that ends the scan stores indptr[batch], the total)
__device__ __forceinline__ void store_page_range(const PlanPageTable& t, int b, int32_t pages_before, int32_t len,
                                                 int32_t np, int32_t page_size) {
  t.indptr[b] = pages_before;
  t.last_page_len[b] = last_page_tokens(len, np, page_size);
}
// fill kernel, workgroup blk of batch x row_blocks: entry j of block-table row b to its place in `indices`, when the
// request has that many pages.  The store is bounded by indptr[b] + j < indptr[batch] <= batch * max_blocks.
__device__ __forceinline__ void compact_page_ids(const PlanRequests& r, const PlanPageTable& t, int blk) {
  const int b = blk / t.row_blocks;
  const int j = (blk - b * t.row_blocks) * kPlanThreads + (int)threadIdx.x;
  const int32_t begin = t.indptr[b];
  if (j < t.indptr[b + 1] - begin) t.indices[begin + j] = r.block_tables[(int64_t)b * r.block_tables_stride + j];
}

// ---- the host side of an entry ----
// The checks come in a fixed order, which a caller cannot change: where two can fail for the same arguments, the one
// made first names the error.

// name_workspace(a, int_bytes, float_bytes): the sizes `layout` computes from host-known values
template <class Args, class Layout>
int plan_workspace_sizes(const char* name, const Args* a, size_t* int_ws_bytes_out, size_t* float_ws_bytes_out,
                         int (*layout)(const Args&, Layout&)) {
  FI_REQUIRE(a && int_ws_bytes_out && float_ws_bytes_out, "%s: null argument", name);
  Layout l;
  if (layout(*a, l)) return 1;
  *int_ws_bytes_out = l.int_bytes;
  *float_ws_bytes_out = l.float_bytes;
  return 0;
}
// the device tensors of an entry (`more`: those beyond the block table, the lengths and the int workspace)
template <class Args>
int check_plan_tensors(const char* name, const Args& a, bool more = true) {
  FI_REQUIRE(a.block_tables && a.seq_lens && a.int_ws && more, "%s: null tensor", name);
  FI_REQUIRE(a.block_tables_stride >= a.max_blocks, "%s: block table rows overlap", name);
  return 0;
}
// both workspaces against what the layout needs; partial states need a float workspace only in a split plan
template <class Args>
int check_plan_workspaces(const char* name, const Args& a, size_t int_bytes, size_t float_bytes, bool split) {
  FI_REQUIRE(int_bytes <= a.int_ws_bytes, "%s: int workspace too small (%zu bytes, need %zu)", name, a.int_ws_bytes,
             int_bytes);
  FI_REQUIRE(float_bytes <= a.float_ws_bytes && (!split || a.float_ws),
             "%s: float workspace too small (%zu bytes, need %zu)", name, a.float_ws_bytes, float_bytes);
  return 0;
}
// the two launches: `scan` on one workgroup, then `fill` on fill_grid of them, on the same stream
template <class Params>
int launch_plan_kernels(void (*scan)(Params), void (*fill)(Params), int64_t fill_grid, const Params& p,
                        fi_stream_t stream) {
  hipLaunchKernelGGL(scan, dim3(1), dim3(kPlanThreads), 0, (hipStream_t)stream, p);
  FI_HIP_CALL(hipGetLastError());
  hipLaunchKernelGGL(fill, dim3((uint32_t)fill_grid), dim3(kPlanThreads), 0, (hipStream_t)stream, p);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}

}  // namespace fi
