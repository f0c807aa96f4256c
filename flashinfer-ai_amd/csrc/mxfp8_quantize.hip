// MXFP8 quantiser: f16 / bf16 rows -> e4m3 values with one E8M0 scale byte per 32 elements.
// ref: cvt_warp_fp16_to_mxfp8, csrc/nv_internal/tensorrt_llm/kernels/quantization.cuh:586-647; Python
// flashinfer/fp8_quantization.py:179-212.
//
// Rule: mx_quant.h, with 448 the largest e4m3 magnitude, the pinned difference from the reference included.
//
// Shape.  One pass with the threads and quads of mx_quant.h (one 16-byte load, one 8-byte store per thread).  The kernel
// is indexed by the rows of the SCALE tensor and by its k blocks, padding included in both (the sizes are
// mx_layout.h's), so that every byte of the scale buffer is written (padding as 0) and the caller needs no memset; a
// row belongs to a row team (common.h).  In the grouped layout a scale row finds its operand row by mx_row_of_scale_row
// (mx_layout.h) on the m_indptr in global memory; the scale rows of no group, also in front of the first, are padding.
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
  int32_t tpr_log2;  // the row team (common.h)
};

template <int DT>
__global__ void __launch_bounds__(kMxQuantThreads) mxfp8_quantize_kernel(const MxQuantArgs A) {
  const RowTeam team = row_team<kMxQuantThreads>(A.tpr_log2, A.items);
  if (team.past_end) return;
  const int64_t item = team.row;

  int src = -1;     // input row, -1: a padding row of the scale tensor
  int64_t s = -1;   // scale row, -1: none (grouped layout, a row past m_indptr[G])
  if (item < A.sf_rows) {
    s = item;
    if (A.m_indptr == nullptr) {
      src = item < A.m ? (int)item : -1;
    } else {
      int group;
      src = mx_row_of_scale_row(A.m_indptr, A.num_groups, s, A.m, group);
    }
  } else {
    // rows of no group (below m_indptr[0], at or past m_indptr[G]) get their q here, without a scale row
    src = (int)(item - A.sf_rows);
    if (src >= A.m_indptr[0] && src < A.m_indptr[A.num_groups]) return;
  }

  const uint16_t* const xr = A.x + (int64_t)max(src, 0) * A.x_stride;
  for (int cc = team.lane; cc < A.nkb_loop * 4; cc += team.size) {
    const int col = cc * 8;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    if (src >= 0 && col < A.k) load_16bit<DT, 8>(xr + col, v);
    const int e = mx_e4m3_exponent(mx_quad_max(mx_amax8(v)));
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
  const int64_t nkb_loop = mx_sf_kblocks(nkb, swizzled);
  const int64_t sf_rows = grouped ? mx_sf_rows_grouped(p->m, p->num_groups) : mx_sf_rows<int64_t>(p->m, swizzled);
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
  a.tpr_log2 = row_team_log2(nkb_loop * 4, kMxQuantThreads);
  const int64_t rows_per_block = kMxQuantThreads >> a.tpr_log2;
  const uint32_t grid = (uint32_t)ceil_div<int64_t>(items, rows_per_block);
  if (p->dtype == FI_DTYPE_F16)
    mxfp8_quantize_kernel<FI_DTYPE_F16><<<dim3(grid), dim3(kMxQuantThreads), 0, (hipStream_t)stream>>>(a);
  else
    mxfp8_quantize_kernel<FI_DTYPE_BF16><<<dim3(grid), dim3(kMxQuantThreads), 0, (hipStream_t)stream>>>(a);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}
