// MXFP4 quantiser and scale interleave: f16 / bf16 rows -> packed e2m1 codes with one E8M0 scale byte per 32 elements,
// and linear scale bytes -> the swizzled "128x4" layout (mx_layout.h).
// ref: cvt_warp_fp16_to_fp4<Type, 32, true>, csrc/nv_internal/tensorrt_llm/kernels/quantization.cuh:427-499;
// block_scale_interleave_kernel, csrc/nv_internal/cpp/kernels/quantization.cu; Python flashinfer/fp4_quantization.py:525-830.
//
// Rule: mx_quant.h, with 6 the largest e2m1 magnitude, the pinned difference from the reference included;
// code = e2m1(x . 2^-e), round to nearest, ties to even.  (In this UE8M0 branch the reference does not use its global
// scale, and neither does this kernel.)
// Two codes share a byte, element 2i in the low nibble of byte i, bit 3 of a code is the sign.
//
// Conversion.  v_cvt_scalef32_pk_fp4_f32 on the values already multiplied by 2^-e, with the instruction's own scale
// operand at 1.0: two f32 -> one byte of two codes.  tools/probe_cvt_fp4.hip records what the instruction does on
// the card.
//
// Shape.  One pass with the threads and quads of mx_quant.h (one 16-byte load, one 4-byte store per thread).  The
// kernel is indexed by the (row, k block) pairs of the SCALE tensor, padding included in both (the sizes are
// mx_layout.h's), so that every byte of the scale buffer is written (padding as 0) and the caller needs no memset.
// The pairs are one flat range, a quad per pair and kMx4Pairs pairs per quad.  (The MXFP8 kernel gives a row to a
// team of threads that loops over the row's blocks; here no lane idles when the blocks of a row do not fill the
// team.)  Every group of `rows` input rows has its own scale rows (swizzled: padded to 128 and swizzled on their own).
#include "common.h"
#include "mx_layout.h"
#include "mx_quant.h"

namespace fi {

constexpr int kMx4QuantThreads = 256;
// (row, k block) pairs per quad.  All their loads are issued before the first is used: with one 16-byte load in
// flight per thread the bytes in flight of a full CU do not cover the HBM latency.
constexpr int kMx4Pairs = 4;
constexpr int kMx4PairsPerWorkgroup = kMx4Pairs * kMx4QuantThreads / 4;

struct Mx4QuantArgs {
  const uint16_t* x;
  uint8_t* q;
  uint8_t* sf;
  int64_t x_stride;
  int64_t sf_group_bytes;  // scale bytes of one group, padding included
  FastDiv nkb_loop;        // k blocks per scale row as written: the swizzled layout pads them to 4
  FastDiv sf_rows;         // scale rows of one group, padding included
  uint32_t blocks;         // num_groups * sf_rows * nkb_loop, < 2^31
  int32_t rows, k;
  int32_t nkb;             // k blocks per row: k / 32
  int32_t swizzled;
};

// one byte: the e2m1 codes of a (low nibble) and b (high nibble); |a|, |b| <= 6
__device__ __forceinline__ uint32_t e2m1_pair(float a, float b) {
  return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(0u, a, b, 1.0f, 0) & 0xffu;
}

template <int DT>
__global__ void __launch_bounds__(kMx4QuantThreads) mxfp4_quantize_kernel(const Mx4QuantArgs A) {
  const uint32_t first = blockIdx.x * kMx4PairsPerWorkgroup + (threadIdx.x >> 2);
  const int lane_col = (threadIdx.x & 3) * 8;
  uint32_t g[kMx4Pairs];
  int s[kMx4Pairs], kb[kMx4Pairs];  // scale row inside the group, k block
  bool live[kMx4Pairs], in[kMx4Pairs];
  float v[kMx4Pairs][8];
#pragma unroll
  for (int u = 0; u < kMx4Pairs; ++u) {
    const uint32_t blk = first + u * (kMx4QuantThreads / 4);
    live[u] = blk < A.blocks;  // whole quads
    const uint32_t item = fast_div(blk, A.nkb_loop);  // scale row, over all groups
    kb[u] = (int)(blk - item * A.nkb_loop.d);
    g[u] = fast_div(item, A.sf_rows);
    s[u] = (int)(item - g[u] * A.sf_rows.d);
    const int col = kb[u] * kMxBlock + lane_col;
    in[u] = live[u] && s[u] < A.rows && col < A.k;  // else padding of the scale tensor
    // no branch around the load (the compiler would wait for it inside): padding reads the first 16 bytes of the input
    load_16bit<DT, 8>(A.x + (in[u] ? ((int64_t)g[u] * A.rows + s[u]) * A.x_stride + col : 0), v[u]);
  }
#pragma unroll
  for (int u = 0; u < kMx4Pairs; ++u) {
    if (!live[u]) continue;
    float amax = mx_amax8(v[u]);
    amax = in[u] ? amax : 0.f;  // a padding lane holds input bytes, not zeros
    const int e = mx_e2m1_exponent(mx_quad_max(amax));
    const float scale = __builtin_bit_cast(float, (uint32_t)(127 - e) << 23);  // 2^-e; e <= 126 for 16-bit inputs
    if (in[u]) {
      uint32_t w = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) w |= e2m1_pair(v[u][2 * j] * scale, v[u][2 * j + 1] * scale) << (8 * j);
      const int64_t src = (int64_t)g[u] * A.rows + s[u];
      *(uint32_t*)(A.q + src * (A.k >> 1) + ((kb[u] * kMxBlock + lane_col) >> 1)) = w;
    }
    if (lane_col == 0) {
      const int64_t pos = A.swizzled ? mx_sf_offset(s[u], kb[u], A.nkb) : (int64_t)s[u] * A.nkb + kb[u];
      A.sf[(int64_t)g[u] * A.sf_group_bytes + pos] = in[u] ? (uint8_t)(e + 127) : (uint8_t)0;
    }
  }
}

struct MxInterleaveArgs {
  const uint8_t* in;
  uint32_t* out;
  int64_t words;        // output dwords: num_groups * group_words
  int32_t group_words;  // pad128(rows) * pad4(cols) / 4
  int32_t k_tiles;      // pad4(cols) / 4
  int32_t rows, cols;
};

// One thread writes one dword of the output: the scales of one row over 4 k blocks (mx_layout.h).
__global__ void __launch_bounds__(256) mx_sf_interleave_kernel(const MxInterleaveArgs A) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= A.words) return;
  const int g = (int)(d / A.group_words);
  const int w = (int)(d - (int64_t)g * A.group_words);
  const int tile = w >> 7, in_tile = w & 127;  // a [128 rows][4 blocks] tile is 128 dwords, [row % 32][row / 32 % 4]
  const int r = (tile / A.k_tiles) * 128 + (in_tile & 3) * 32 + (in_tile >> 2);
  const int kb0 = (tile % A.k_tiles) * 4;
  uint32_t word = 0;
  if (r < A.rows) {
    const uint8_t* const p = A.in + ((int64_t)g * A.rows + r) * A.cols;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (kb0 + j < A.cols) word |= (uint32_t)p[kb0 + j] << (8 * j);
  }
  A.out[d] = word;
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_mxfp4_quantize(const fi_mxfp4_quantize_params_t* p, fi_stream_t stream) {
  FI_REQUIRE(p, "mxfp4_quantize: null params");
  FI_REQUIRE(p->num_groups >= 0 && p->rows >= 0 && p->k >= 0, "mxfp4_quantize: negative size (num_groups %d, rows %d, k %d)",
             p->num_groups, p->rows, p->k);
  FI_REQUIRE(p->k % kMxBlock == 0, "mxfp4_quantize: k %d must be a multiple of 32", p->k);
  FI_REQUIRE(p->k < (1 << 30), "mxfp4_quantize: k too large");
  FI_REQUIRE(p->dtype == FI_DTYPE_F16 || p->dtype == FI_DTYPE_BF16, "mxfp4_quantize: dtype %d is not f16 or bf16", p->dtype);
  FI_REQUIRE(p->sf_layout == FI_MX_SF_LINEAR || p->sf_layout == FI_MX_SF_SWIZZLED_128X4,
             "mxfp4_quantize: unknown scale layout %d", p->sf_layout);
  const bool swizzled = p->sf_layout == FI_MX_SF_SWIZZLED_128X4;
  const int64_t nkb = p->k / kMxBlock;
  const int64_t nkb_loop = mx_sf_kblocks(nkb, swizzled);
  const int64_t sf_rows = mx_sf_rows<int64_t>(p->rows, swizzled);
  const int64_t items = sf_rows * p->num_groups;
  if (items == 0 || nkb_loop == 0) return 0;
  FI_REQUIRE(items < (1ll << 31), "mxfp4_quantize: too many rows");
  const int64_t blocks = items * nkb_loop;  // one scale byte each
  FI_REQUIRE(blocks < (1ll << 31), "mxfp4_quantize: the scale tensor would hold %lld bytes, 2^31 or more", (long long)blocks);
  FI_REQUIRE(p->input && p->q && p->sf, "mxfp4_quantize: null tensor");
  FI_REQUIRE(p->input_stride >= p->k, "mxfp4_quantize: input stride %lld is smaller than k %d", (long long)p->input_stride,
             p->k);
  FI_REQUIRE(((uintptr_t)p->input % 16) == 0 && p->input_stride % 8 == 0 && ((uintptr_t)p->q % 4) == 0,
             "mxfp4_quantize: input must be 16-byte aligned with a row stride that is a multiple of 8, q 4-byte aligned");
  FI_REQUIRE(p->sf_bytes >= blocks, "mxfp4_quantize: sf holds %lld bytes, %lld needed", (long long)p->sf_bytes,
             (long long)blocks);
  Mx4QuantArgs a{};
  a.x = (const uint16_t*)p->input;
  a.q = (uint8_t*)p->q;
  a.sf = (uint8_t*)p->sf;
  a.x_stride = p->input_stride;
  a.sf_group_bytes = sf_rows * nkb_loop;
  a.nkb_loop = FastDiv((uint32_t)nkb_loop);
  a.sf_rows = FastDiv((uint32_t)sf_rows);
  a.blocks = (uint32_t)blocks;
  a.rows = p->rows;
  a.k = p->k;
  a.nkb = (int32_t)nkb;
  a.swizzled = swizzled;
  const uint32_t grid = (uint32_t)ceil_div<int64_t>(blocks, kMx4PairsPerWorkgroup);
  if (p->dtype == FI_DTYPE_F16)
    mxfp4_quantize_kernel<FI_DTYPE_F16><<<dim3(grid), dim3(kMx4QuantThreads), 0, (hipStream_t)stream>>>(a);
  else
    mxfp4_quantize_kernel<FI_DTYPE_BF16><<<dim3(grid), dim3(kMx4QuantThreads), 0, (hipStream_t)stream>>>(a);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}

extern "C" FI_API int fi_mx_sf_interleave(const fi_mx_sf_interleave_params_t* p, fi_stream_t stream) {
  FI_REQUIRE(p, "mx_sf_interleave: null params");
  FI_REQUIRE(p->num_groups >= 0 && p->rows >= 0 && p->cols >= 0,
             "mx_sf_interleave: negative size (num_groups %d, rows %d, cols %d)", p->num_groups, p->rows, p->cols);
  const int64_t k_tiles = mx_sf_kblocks<int64_t>(p->cols, true) / 4;
  const int64_t group_words = mx_sf_rows<int64_t>(p->rows, true) * k_tiles;
  if (group_words == 0 || p->num_groups == 0) return 0;
  FI_REQUIRE(group_words < (1ll << 31), "mx_sf_interleave: tensor too large");
  const int64_t words = group_words * p->num_groups;
  FI_REQUIRE(words < (1ll << 38), "mx_sf_interleave: tensor too large");
  FI_REQUIRE(p->input && p->output, "mx_sf_interleave: null tensor");
  FI_REQUIRE(((uintptr_t)p->output % 4) == 0, "mx_sf_interleave: output must be 4-byte aligned");
  FI_REQUIRE(p->output_bytes >= words * 4, "mx_sf_interleave: output holds %lld bytes, %lld needed", (long long)p->output_bytes,
             (long long)(words * 4));
  MxInterleaveArgs a{};
  a.in = (const uint8_t*)p->input;
  a.out = (uint32_t*)p->output;
  a.words = words;
  a.group_words = (int32_t)group_words;
  a.k_tiles = (int32_t)k_tiles;
  a.rows = p->rows;
  a.cols = p->cols;
  mx_sf_interleave_kernel<<<dim3((uint32_t)ceil_div<int64_t>(words, 256)), dim3(256), 0, (hipStream_t)stream>>>(a);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}
