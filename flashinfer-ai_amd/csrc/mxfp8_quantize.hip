// MXFP8 quantiser: f16 / bf16 rows -> e4m3 values with one E8M0 scale byte per 32 elements.
// ref: cvt_warp_fp16_to_mxfp8, csrc/nv_internal/tensorrt_llm/kernels/quantization.cuh:586-647; Python
// flashinfer/fp8_quantization.py:179-212.
//
// Rule (the device code is mx_quant.h, shared with the MoE layer's gated activation).  Per block of 32: amax = max |x|;
// e = the smallest integer in [-127, 127] with 448 . 2^e >= amax (amax = 0: e = -127); scale byte = e + 127;
// q = e4m3(x . 2^-e), round to nearest even.  The multiplication by a power of two is exact and |x . 2^-e| <= 448, so
// the conversion never saturates.  (The reference multiplies by an approximate reciprocal of 448 and rounds the
// quotient's exponent up; at amax exactly 448 . 2^e its hardware may give e + 1.  The compare here is exact: see
// fi_mi355.h.)
//
// Shape.  One pass: a thread owns 8 consecutive elements (one 16-byte load, one 8-byte store), the 4 threads of a
// block of 32 are the 4 lanes of a quad and share amax by two quad-permute moves.  The kernel is indexed by the rows
// of the SCALE tensor, padding included, and by its k blocks, padding included, so that every byte of the scale
// buffer is written (padding as 0) and the caller needs no memset.  In the grouped layout (mx_layout.h) a scale
// row finds its group by a binary search over m_indptr on the device.
#include <algorithm>

#include "common.h"
#include "mx_layout.h"
#include "mx_quant.h"

namespace fi {

constexpr int kMxQuantThreads = 256;

struct MxQuantArgs {
  const uint16_t* x;
  uint8_t* q;
  uint8_t* sf;
  const int32_t* m_indptr;  // grouped layout: [num_groups + 1] device
  int64_t x_stride;
  int32_t m, k, k_pad;
  int32_t nkb;       // k blocks per scale row as the offset function takes them: k_pad / 32
  int32_t nkb_loop;  // ... as written: the swizzled layouts pad them to 4
  int32_t sf_rows;   // rows of the scale tensor, padding included
  int32_t items;     // sf_rows, plus m for the grouped layout (rows outside every group still get their q)
  int32_t num_groups;
  int32_t swizzled;
  int32_t tpr_log2;  // threads per row
};

template <int DT>
__global__ void __launch_bounds__(kMxQuantThreads) mxfp8_quantize_kernel(const MxQuantArgs A) {
  const int tpr = 1 << A.tpr_log2;
  const int t = threadIdx.x & (tpr - 1);
  const int64_t item = (int64_t)blockIdx.x * (kMxQuantThreads >> A.tpr_log2) + (threadIdx.x >> A.tpr_log2);
  if (item >= A.items) return;  // whole quads leave: tpr is a multiple of 4

  int src = -1;     // input row, -1: a padding row of the scale tensor
  int64_t s = -1;   // scale row, -1: none (grouped layout, a row past m_indptr[G])
  if (item < A.sf_rows) {
    s = item;
    if (A.m_indptr == nullptr) {
      src = item < A.m ? (int)item : -1;
    } else {
      int lo = 0, hi = A.num_groups;  // invariant: first scale row of lo <= s (< first scale row of hi)
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (mx_sf_row_offset(A.m_indptr[mid], mid) <= s) lo = mid; else hi = mid;
      }
      const int begin = A.m_indptr[lo], end = A.m_indptr[lo + 1];
      const int64_t r = s - mx_sf_row_offset(begin, lo);
      src = (begin >= 0 && r < (int64_t)end - begin && begin + r < A.m) ? (int)(begin + r) : -1;
    }
  } else {
    // rows of no group (below m_indptr[0], at or past m_indptr[G]) get their q here, without a scale row
    src = (int)(item - A.sf_rows);
    if (src >= A.m_indptr[0] && src < A.m_indptr[A.num_groups]) return;
  }

  const uint16_t* const xr = A.x + (int64_t)max(src, 0) * A.x_stride;
  for (int cc = t; cc < A.nkb_loop * 4; cc += tpr) {
    const int col = cc * 8;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    if (src >= 0 && col < A.k) load_16bit<DT, 8>(xr + col, v);
    const int e = mx_e4m3_exponent(mx_quad_amax(v));
    if (src >= 0 && col < A.k_pad) *(u32x2*)(A.q + (int64_t)src * A.k_pad + col) = mx_e4m3_pack8(v, e);
    if (s >= 0 && (cc & 3) == 0) {
      const int kb = cc >> 2;
      const int64_t pos = A.swizzled ? mx_sf_offset((int)s, kb, A.nkb) : s * A.nkb + kb;
      A.sf[pos] = (src >= 0 && col < A.k) ? (uint8_t)(e + 127) : (uint8_t)0;
    }
  }
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_mxfp8_quantize(const fi_mxfp8_quantize_params_t* p, fi_stream_t stream) {
  FI_REQUIRE(p, "mxfp8_quantize: null params");
  FI_REQUIRE(p->m >= 0 && p->k >= 0 && p->num_groups >= 0, "mxfp8_quantize: negative size (m %d, k %d, num_groups %d)",
             p->m, p->k, p->num_groups);
  FI_REQUIRE(p->k % kMxBlock == 0, "mxfp8_quantize: k %d must be a multiple of 32", p->k);
  FI_REQUIRE(p->alignment > 0 && p->alignment % kMxBlock == 0, "mxfp8_quantize: alignment %d must be a positive multiple of 32",
             p->alignment);
  FI_REQUIRE(p->dtype == FI_DTYPE_F16 || p->dtype == FI_DTYPE_BF16, "mxfp8_quantize: dtype %d is not f16 or bf16", p->dtype);
  FI_REQUIRE(p->sf_layout == FI_MX_SF_LINEAR || p->sf_layout == FI_MX_SF_SWIZZLED_128X4,
             "mxfp8_quantize: unknown scale layout %d", p->sf_layout);
  const bool grouped = p->m_indptr != nullptr;
  FI_REQUIRE(!grouped || (p->sf_layout == FI_MX_SF_SWIZZLED_128X4 && p->num_groups > 0),
             "mxfp8_quantize: the grouped layout (m_indptr) is swizzled and needs num_groups > 0");
  const int64_t k_pad = ceil_div<int64_t>(p->k, p->alignment) * p->alignment;
  FI_REQUIRE(k_pad < (1ll << 30), "mxfp8_quantize: k too large");
  const bool swizzled = p->sf_layout == FI_MX_SF_SWIZZLED_128X4;
  const int64_t nkb = k_pad / kMxBlock;
  const int64_t nkb_loop = swizzled ? ceil_div<int64_t>(nkb, 4) * 4 : nkb;
  const int64_t sf_rows = grouped ? mx_sf_row_offset(p->m, p->num_groups)
                                  : (swizzled ? ceil_div<int64_t>(p->m, 128) * 128 : (int64_t)p->m);
  const int64_t items = sf_rows + (grouped ? p->m : 0);
  if (items == 0 || k_pad == 0) return 0;
  FI_REQUIRE(sf_rows < (1ll << 31) && items < (1ll << 31), "mxfp8_quantize: too many rows");
  FI_REQUIRE(p->sf, "mxfp8_quantize: null tensor (sf)");
  FI_REQUIRE(p->m == 0 || (p->input && p->q), "mxfp8_quantize: null tensor");
  FI_REQUIRE(p->input_stride >= p->k, "mxfp8_quantize: input stride %lld is smaller than k %d", (long long)p->input_stride,
             p->k);
  FI_REQUIRE(((uintptr_t)p->input % 16) == 0 && p->input_stride % 8 == 0 && ((uintptr_t)p->q % 8) == 0,
             "mxfp8_quantize: input must be 16-byte aligned with a row stride that is a multiple of 8, q 8-byte aligned");
  FI_REQUIRE(p->sf_bytes >= sf_rows * nkb_loop, "mxfp8_quantize: sf holds %lld bytes, %lld needed", (long long)p->sf_bytes,
             (long long)(sf_rows * nkb_loop));
  MxQuantArgs a{};
  a.x = (const uint16_t*)p->input;
  a.q = (uint8_t*)p->q;
  a.sf = (uint8_t*)p->sf;
  a.m_indptr = p->m_indptr;
  a.x_stride = p->input_stride;
  a.m = p->m;
  a.k = p->k;
  a.k_pad = (int32_t)k_pad;
  a.nkb = (int32_t)nkb;
  a.nkb_loop = (int32_t)nkb_loop;
  a.sf_rows = (int32_t)sf_rows;
  a.items = (int32_t)items;
  a.num_groups = p->num_groups;
  a.swizzled = swizzled;
  // threads per row: a power of two from one quad to the workgroup, enough for the row's chunks when it can be
  int tpr_log2 = 2;
  while ((1 << tpr_log2) < kMxQuantThreads && (1ll << tpr_log2) < nkb_loop * 4) ++tpr_log2;
  a.tpr_log2 = tpr_log2;
  const int64_t rows_per_block = kMxQuantThreads >> tpr_log2;
  const uint32_t grid = (uint32_t)ceil_div<int64_t>(items, rows_per_block);
  if (p->dtype == FI_DTYPE_F16)
    mxfp8_quantize_kernel<FI_DTYPE_F16><<<dim3(grid), dim3(kMxQuantThreads), 0, (hipStream_t)stream>>>(a);
  else
    mxfp8_quantize_kernel<FI_DTYPE_BF16><<<dim3(grid), dim3(kMxQuantThreads), 0, (hipStream_t)stream>>>(a);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}
