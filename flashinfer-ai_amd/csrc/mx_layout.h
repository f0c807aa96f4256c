// Where the E8M0 scale bytes of an MX operand live: the one place the quantiser (mxfp8_quantize.hip) and the MXFP4
// grouped GEMM (gemm_mxfp4.hip) share.  One scale byte covers 32 consecutive k elements of one row.
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

// first scale row of group g whose first operand row is m_begin; with (cum_m, G) the row count of the whole tensor
FI_MX_HD int64_t mx_sf_row_offset(int64_t m_begin, int64_t g) { return (m_begin + g * 127) / 128 * 128; }

}  // namespace fi
