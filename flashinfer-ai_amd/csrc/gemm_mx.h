// Shared by the translation units on the block-scaled 16x16x128 MFMA (gemm_mxfp4.hip, mm_fp4.hip): the MFMA step and
// its operands, the masked store of a lane's result, the token tile choice and the host checks both entry points make.
// The lane maps are in the headers of the two files.
#pragma once
#include <type_traits>

#include "gemm_common.h"
#include "mx_layout.h"

namespace fi {

// a lane's 16 bytes of an fp4 operand (32 e2m1 codes) in the first 4 of the operand's 8 registers
__device__ __forceinline__ i32x8g mx_fp4_frag(const u32x4& v) {
  return i32x8g{(int)v[0], (int)v[1], (int)v[2], (int)v[3], 0, 0, 0, 0};
}
// the lane's k block q out of a row's dword of four E8M0 scales
__device__ __forceinline__ int mx_scale_byte(uint32_t s, int q) { return (int)((s >> (8 * q)) & 0xffu); }

// One block-scaled step: acc + 16 weight rows (fw: fp4, cbsz 4; exponent ew) x 16 tokens (fx, ex) over 128 k.  BLGP is
// the token operand's format: 0 e4m3, 1 e5m2, 4 fp4.  The fragments and exponents come prepared, so that a kernel
// builds a weight block's once for all its token blocks: built in here per call, the grouped kernel's MB = 2 k loop
// grew from 76 to 87 instructions (twelve v_accvgpr moves) and 100 to 108 VGPRs.
template <int BLGP>
__device__ __forceinline__ f32x4 mx_mfma(const i32x8g& fw, int ew, const i32x8g& fx, int ex, const f32x4& acc) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, fx, acc, /*cbsz fp4*/ 4, BLGP, 0, ew, 0, ex);
}

// A lane's 4 consecutive n of token row m, times alpha: 8 bytes of d (rows of N), masked past m_end and N.  n and N
// are multiples of 4 resp. 8, so a piece is inside n or outside it as a whole.
__device__ __forceinline__ void mx_store_piece(void* d, int out_dtype, int m, int m_end, int n, int N, const f32x4& v,
                                               float alpha) {
  if (m >= m_end || n >= N) return;
  // element by element: the f16 conversion then takes the product in one instruction (v_fma_mixlo_f16, one rounding);
  // as a vector product it is rounded to f32 first, and results with alpha differ in the last bit
  *(u32x2*)((uint16_t*)d + (int64_t)m * N + n) = u32x2{pack_16bit(v[0] * alpha, v[1] * alpha, out_dtype),
                                                       pack_16bit(v[2] * alpha, v[3] * alpha, out_dtype)};
}

// go(std::integral_constant<int, MB>) for a token tile of MB 16-row blocks: 1, 2 or 4, a tile that `rows` fill
template <class F>
void with_mx_token_blocks(int64_t rows, F&& go) {
  if (rows <= 16) go(std::integral_constant<int, 1>{});
  else if (rows <= 32) go(std::integral_constant<int, 2>{});
  else go(std::integral_constant<int, 4>{});
}

// The checks fi_group_gemm_mxfp8_mxfp4_nt_groupwise and fi_mm_mxfp4 share, in their order.  align_what, a_rows and
// b_rows are the entry point's words for what it asks; b_need covers b_tensors weight tensors of equal size.
inline int mx_check_common(const char* who, int d_dtype, int n, int k, bool aligned, const char* align_what,
                           int64_t a_scale_bytes, int64_t a_need, const char* a_rows, int64_t b_scale_bytes,
                           int64_t b_need, int b_tensors, const char* b_rows, int64_t tiles) {
  FI_REQUIRE(d_dtype == FI_DTYPE_F16 || d_dtype == FI_DTYPE_BF16, "%s: output dtype %d is not f16 / bf16", who, d_dtype);
  FI_REQUIRE(n % 8 == 0, "%s: n %d must be a multiple of 8", who, n);
  FI_REQUIRE(k > 0 && k % 128 == 0, "%s: k %d must be a positive multiple of 128", who, k);
  FI_REQUIRE(aligned, "%s: a / b must be 16-byte, %s aligned", who, align_what);
  FI_REQUIRE(a_scale_bytes >= a_need, "%s: a_scale holds %lld bytes, %lld needed (%s)", who, (long long)a_scale_bytes,
             (long long)a_need, a_rows);
  FI_REQUIRE(b_scale_bytes >= b_need, "%s: b_scale holds %lld bytes, %lld needed (%s)", who, (long long)b_scale_bytes,
             (long long)b_need, b_rows);
  // 32-bit offsets inside a tile and inside a scale tensor
  FI_REQUIRE(a_need < (1ll << 31) && b_need / b_tensors < (1ll << 31) && (int64_t)k * 128 < (1ll << 31),
             "%s: problem too large for 32-bit tile offsets", who);
  FI_REQUIRE(tiles < (1ll << 31), "%s: too many tiles", who);
  return 0;
}

}  // namespace fi
