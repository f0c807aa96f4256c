// Where the E8M0 scale bytes of an MX operand live and how many there are: the one place the quantisers
// (mxfp8_quantize.hip, mxfp4_quantize.hip), the MXFP4 grouped GEMM (gemm_mxfp4.hip) and the MoE stages (moe.hip) share;
// flashinfer/_mx.py is the Python side.  One scale byte covers 32 consecutive k elements of one row.
//
// Swizzled "128x4" layout (ref: get_sf_out_offset_128x4, csrc/nv_internal/tensorrt_llm/kernels/quantization.cuh:649-688):
// rows pad to 128, k blocks to 4; a [128 rows][4 blocks] tile is 512 bytes, stored as [row % 32][(row % 128) / 32][kb % 4].
// The four scales of a row over 128 k elements are therefore one aligned dword, and 16 bytes hold those dwords for
// rows r, r + 32, r + 64, r + 96.
//
// Grouped placement (ref: compute_sm100_cutlass_group_gemm_args, include/flashinfer/gemm/
// group_gemm_mxfp4_groupwise_sm100.cuh:54-90): the scale rows of group g of the row operand start at scale row
// mx_sf_row_offset(m_indptr[g], g), a multiple of 128, and are swizzled on their own from there; the scales of
// group g of the (n, k) operand start at byte g * ceil(n / 128) * 128 * (k / 32).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FI_MX_HD __host__ __device__ __forceinline__
#else
#define FI_MX_HD inline
#endif

namespace fi {

constexpr int kMxBlock = 32;  // k elements per scale byte

// byte of (row r, k block kb) in a swizzled scale tensor of nkb k blocks per row
FI_MX_HD int64_t mx_sf_offset(int r, int kb, int nkb) {
  const int k_tiles = (nkb + 3) >> 2;
  return ((int64_t)(r >> 7) * k_tiles + (kb >> 2)) * 512 + (r & 31) * 16 + ((r & 127) >> 5) * 4 + (kb & 3);
}

// first scale row of group g whose first operand row is m_begin
FI_MX_HD int64_t mx_sf_row_offset(int64_t m_begin, int64_t g) { return (m_begin + g * 127) / 128 * 128; }

// rows and k blocks of a scale tensor as stored, padding included; the grouped layout ends where a group G would begin
template <typename T>
FI_MX_HD T mx_sf_rows(T m, bool swizzled) { return swizzled ? (m + 127) / 128 * 128 : m; }
FI_MX_HD int64_t mx_sf_rows_grouped(int64_t cum_m, int64_t G) { return mx_sf_row_offset(cum_m, G); }
template <typename T>
FI_MX_HD T mx_sf_kblocks(T nkb, bool swizzled) { return swizzled ? (nkb + 3) / 4 * 4 : nkb; }

// group of scale row s of the grouped layout and the operand row it holds (-1: a padding row, also one in front of the
// first group or of a row at or past cum_m); m_indptr (G + 1 entries) is in global memory or a copy in LDS
FI_MX_HD int mx_row_of_scale_row(const int32_t* m_indptr, int G, int64_t s, int cum_m, int& group) {
  int lo = 0, hi = G;  // invariant: first scale row of lo <= s (< first scale row of hi)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (mx_sf_row_offset(m_indptr[mid], mid) <= s) lo = mid; else hi = mid;
  }
  group = lo;
  const int begin = m_indptr[lo], end = m_indptr[lo + 1];
  const int64_t r = s - mx_sf_row_offset(begin, lo);
  return (begin >= 0 && r >= 0 && r < (int64_t)end - begin && begin + r < cum_m) ? (int)(begin + r) : -1;
}

}  // namespace fi
