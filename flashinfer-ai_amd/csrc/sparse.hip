// Block-sparse index plumbing: a per-head block map over variable-size column blocks -> the page table the attention
// kernels read, and block-sparse indices -> per-token offsets.
// ref: _block_mask_map_to_expanded_indices flashinfer/sparse.py:929-974 (a chain of torch ops there);
//      BlockSparseIndicesToVectorSparseOffsetsKernel include/flashinfer/page.cuh:287-302.
// All three kernels are bound by their int32 stores: consecutive lanes write consecutive entries.
#include <algorithm>

#include "common.h"

namespace fi {

constexpr int kSparseThreads = 256;
constexpr int kSparseWaves = kSparseThreads / 64;

// one workgroup per (head, block row): pages its selected column blocks hold
__global__ void __launch_bounds__(kSparseThreads)
    block_mask_row_pages_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ col_sz,
                                int32_t* __restrict__ row_pages, int MB, int NB, FastDiv granule) {
  __shared__ int wave_total[kSparseWaves];
  const int row = blockIdx.x, h = row / MB;
  const uint8_t* m = mask + (int64_t)row * NB;
  const int32_t* cs = col_sz + (int64_t)h * NB;
  int pages = 0;
  for (int c = threadIdx.x; c < NB; c += kSparseThreads)
    if (m[c]) pages += (int)fast_div((uint32_t)cs[c], granule);
  const int total = block_reduce<kSparseWaves, RedSum>(pages, wave_total);
  if (threadIdx.x == 0) row_pages[row] = total;
}

// One workgroup per (head, block row), kSparseThreads column blocks at a time.  Two scans over the columns give every
// block its first page (all blocks counted) and the offset of its pages in the row's output (selected blocks counted);
// both go to LDS, and the threads then walk the output positions of these columns, each finding its block by a
// binary search over the offsets: a block of any size is written by consecutive lanes.
__global__ void __launch_bounds__(kSparseThreads)
    block_mask_to_page_indices_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ col_sz,
                                      const int32_t* __restrict__ kv_indptr, int32_t* __restrict__ kv_indices, int MB,
                                      int NB, FastDiv granule, int64_t head_pages, int64_t capacity) {
  __shared__ int wave_total[kSparseWaves];
  __shared__ int out_end[kSparseThreads];  // end of the block's pages among this pass's output positions
  __shared__ int page_of[kSparseThreads];  // page number = page_of[block] + output position
  const int row = blockIdx.x, h = row / MB;
  const uint8_t* m = mask + (int64_t)row * NB;
  const int32_t* cs = col_sz + (int64_t)h * NB;
  int first_page = (int)((int64_t)h * head_pages);  // of the pass's first column; < 2^31, checked on the host
  int64_t out = kv_indptr[row];
  const int64_t row_end = kv_indptr[row + 1];
  const int64_t out_limit = row_end < capacity ? row_end : capacity;
  for (int c0 = 0; c0 < NB; c0 += kSparseThreads) {
    const int c = c0 + threadIdx.x;
    const int pages = c < NB ? (int)fast_div((uint32_t)cs[c], granule) : 0;
    const int emitted = (c < NB && m[c]) ? pages : 0;
    int pass_pages, pass_emitted;
    // the scans' barriers also stand between the previous pass's reads of out_end / page_of and the writes below
    const int pages_incl = block_incl_scan<kSparseWaves>(pages, wave_total, pass_pages);
    const int emitted_incl = block_incl_scan<kSparseWaves>(emitted, wave_total, pass_emitted);
    out_end[threadIdx.x] = emitted_incl;
    page_of[threadIdx.x] = first_page + (pages_incl - pages) - (emitted_incl - emitted);
    __syncthreads();
    for (int p = threadIdx.x; p < pass_emitted; p += kSparseThreads) {
      int lo = 0, hi = kSparseThreads - 1;  // first block whose pages end past p
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (out_end[mid] > p) hi = mid; else lo = mid + 1;
      }
      if (out >= 0 && out + p < out_limit) kv_indices[out + p] = page_of[lo] + p;
    }
    first_page += pass_pages;
    out += pass_emitted;
  }
}

// requests strided over the grid (the reference's loop steps ++b: every workgroup redoes every later request)
__global__ void __launch_bounds__(kSparseThreads)
    block_sparse_to_vector_sparse_kernel(const int32_t* __restrict__ block_indices,
                                         const int32_t* __restrict__ block_indptr, int32_t* __restrict__ offsets,
                                         const int32_t* __restrict__ vector_indptr,
                                         const int32_t* __restrict__ kv_lens, int32_t stride_block, int32_t stride_n,
                                         int batch_size, FastDiv block_div, int block_size, int64_t num_indices,
                                         int64_t capacity) {
  for (int b = blockIdx.x; b < batch_size; b += gridDim.x) {
    const int len = kv_lens[b];
    const int64_t in = block_indptr[b], out = vector_indptr[b];
    if (in < 0 || out < 0) continue;
    for (int pos = threadIdx.x; pos < len; pos += kSparseThreads) {
      const int q = (int)fast_div((uint32_t)pos, block_div);
      const int r = pos - q * block_size;
      if (in + q < num_indices && out + pos < capacity)
        offsets[out + pos] = block_indices[in + q] * stride_block + r * stride_n;
    }
  }
}

static int check_block_map(const char* what, const void* mask, const void* col_sz, int32_t H, int32_t MB, int32_t NB,
                           int32_t granule, int64_t kv_len) {
  FI_REQUIRE(mask && col_sz, "%s: null tensor", what);
  FI_REQUIRE(H > 0 && MB > 0 && NB > 0, "%s: bad block map shape [%d, %d, %d]", what, H, MB, NB);
  FI_REQUIRE((int64_t)H * MB < (1ll << 31), "%s: %d heads x %d block rows exceed the grid", what, H, MB);
  FI_REQUIRE(granule > 0 && kv_len >= 0 && kv_len % granule == 0,
             "%s: granule %d must be positive and divide kv_len %lld", what, granule, (long long)kv_len);
  FI_REQUIRE(kv_len / granule <= ((1ll << 31) - 1) / H,
             "%s: %d heads x %lld pages do not fit int32 page numbers", what, H, (long long)(kv_len / granule));
  return 0;
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_block_mask_row_pages(const uint8_t* block_mask_map, const int32_t* block_col_sz,
                                              int32_t num_heads, int32_t num_block_rows, int32_t num_block_cols,
                                              int32_t granule, int64_t kv_len, int32_t* row_pages,
                                              fi_stream_t stream) {
  if (int rc = check_block_map("block_mask_row_pages", block_mask_map, block_col_sz, num_heads, num_block_rows,
                               num_block_cols, granule, kv_len))
    return rc;
  FI_REQUIRE(row_pages, "block_mask_row_pages: null output");
  block_mask_row_pages_kernel<<<dim3(num_heads * num_block_rows), dim3(kSparseThreads), 0, (hipStream_t)stream>>>(
      block_mask_map, block_col_sz, row_pages, num_block_rows, num_block_cols, FastDiv((uint32_t)granule));
  FI_HIP_CALL(hipGetLastError());
  return 0;
}

extern "C" FI_API int fi_block_mask_to_page_indices(const uint8_t* block_mask_map, const int32_t* block_col_sz,
                                                    const int32_t* kv_indptr, int32_t num_heads,
                                                    int32_t num_block_rows, int32_t num_block_cols, int32_t granule,
                                                    int64_t kv_len, int64_t num_pages, int64_t capacity,
                                                    int32_t* kv_indices, fi_stream_t stream) {
  if (int rc = check_block_map("block_mask_to_page_indices", block_mask_map, block_col_sz, num_heads, num_block_rows,
                               num_block_cols, granule, kv_len))
    return rc;
  FI_REQUIRE(kv_indptr, "block_mask_to_page_indices: null kv_indptr");
  FI_REQUIRE(num_pages >= 0 && num_pages < (1ll << 31),
             "block_mask_to_page_indices: %lld pages do not fit an int32 kv_indptr", (long long)num_pages);
  FI_REQUIRE(capacity >= num_pages, "block_mask_to_page_indices: kv_indices holds %lld entries, the map selects %lld",
             (long long)capacity, (long long)num_pages);
  if (num_pages == 0) return 0;
  FI_REQUIRE(kv_indices, "block_mask_to_page_indices: null kv_indices");
  block_mask_to_page_indices_kernel<<<dim3(num_heads * num_block_rows), dim3(kSparseThreads), 0,
                                      (hipStream_t)stream>>>(
      block_mask_map, block_col_sz, kv_indptr, kv_indices, num_block_rows, num_block_cols,
      FastDiv((uint32_t)granule), kv_len / granule, capacity);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}

extern "C" FI_API int fi_block_sparse_indices_to_vector_sparse_offsets(
    const int32_t* block_sparse_indices, const int32_t* block_sparse_indptr, int32_t* vector_sparse_offsets,
    const int32_t* vector_sparse_indptr, const int32_t* kv_lens, int64_t stride_block, int64_t stride_n,
    int32_t batch_size, int32_t block_size, int64_t num_indices, int64_t capacity, fi_stream_t stream) {
  FI_REQUIRE(batch_size >= 0 && block_size > 0, "block_sparse_indices_to_vector_sparse_offsets: bad batch size %d or "
             "block size %d", batch_size, block_size);
  if (batch_size == 0) return 0;
  FI_REQUIRE(block_sparse_indices && block_sparse_indptr && vector_sparse_offsets && vector_sparse_indptr && kv_lens,
             "block_sparse_indices_to_vector_sparse_offsets: null tensor");
  FI_REQUIRE(stride_block >= 0 && stride_n >= 0 && stride_block < (1ll << 31) && stride_n < (1ll << 31),
             "block_sparse_indices_to_vector_sparse_offsets: strides %lld / %lld do not fit int32 offsets",
             (long long)stride_block, (long long)stride_n);
  FI_REQUIRE(num_indices >= 0 && capacity >= 0, "block_sparse_indices_to_vector_sparse_offsets: negative size");
  const int grid = std::min(batch_size, 256 * 8);
  block_sparse_to_vector_sparse_kernel<<<dim3(grid), dim3(kSparseThreads), 0, (hipStream_t)stream>>>(
      block_sparse_indices, block_sparse_indptr, vector_sparse_offsets, vector_sparse_indptr, kv_lens,
      (int32_t)stride_block, (int32_t)stride_n, batch_size, FastDiv((uint32_t)block_size), block_size, num_indices,
      capacity);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}
