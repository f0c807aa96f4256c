// The MXFP8 quantisation rule as device code: what the quantiser (mxfp8_quantize.hip) and the gated activation of the
// MoE layer (moe.hip) share, so that both produce the same bytes for the same f32 values.
//
// Per block of 32: amax = max |x|; e = the smallest integer in [-127, 127] with 448 . 2^e >= amax (amax = 0: e = -127);
// scale byte = e + 127; q = e4m3(x . 2^-e), round to nearest even.  e is read off the f32 bits of amax = f . 2^E,
// 1 <= f < 2: 448 = 1.75 . 2^8, so e = E - 8 when f <= 1.75 (mantissa field <= 0x600000) and E - 7 otherwise -- an
// integer compare, no log2.  A thread owns 8 consecutive elements; the 4 threads of a block are the 4 lanes of a quad.
#pragma once
#include "common.h"

#if defined(__HIPCC__)
namespace fi {

// amax of a block of 32 from the 8 values of every lane of its quad
__device__ __forceinline__ float mx_quad_amax(const float* v) {
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
  amax = fmaxf(amax, lane_xor<1>(amax));
  return fmaxf(amax, lane_xor<2>(amax));
}

// the block's scale exponent e
__device__ __forceinline__ int mx_e4m3_exponent(float amax) {
  const uint32_t bits = __builtin_bit_cast(uint32_t, amax);
  const int e = (int)(bits >> 23) - 127 - 8 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
  return min(max(e, -127), 127);
}

// 8 values times 2^-e as 8 e4m3 bytes; e <= 120 for every finite f32 amax, so 2^-e is a normal f32
__device__ __forceinline__ u32x2 mx_e4m3_pack8(const float* v, int e) {
  const float scale = __builtin_bit_cast(float, (uint32_t)(127 - e) << 23);
  uint32_t w[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = __builtin_amdgcn_fmed3f(v[4 * h + j] * scale, -448.f, 448.f);
    int packed = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
    packed = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], packed, true);
    w[h] = (uint32_t)packed;
  }
  return u32x2{w[0], w[1]};
}

}  // namespace fi
#endif  // __HIPCC__
