// The MX quantisation rule as device code, for both element formats: what the MXFP8 quantiser (mxfp8_quantize.hip), the
// gated activation of the MoE layer (moe.hip) and the MXFP4 quantiser (mxfp4_quantize.hip) share, so that all produce
// the same scale byte for the same f32 values.
//
// Per block of 32: amax = max |x|; e = the smallest integer in [-127, 127] with qmax . 2^e >= amax (amax = 0: e = -127),
// qmax the format's largest magnitude; scale byte = e + 127; q = x . 2^-e in the format, round to nearest even.  e is
// read off the f32 bits of amax = f . 2^E, 1 <= f < 2: with qmax = c . 2^P, 1 <= c < 2, e = E - P when f <= c (mantissa
// field <= that of c) and E - P + 1 otherwise -- an integer compare, no log2.  e4m3: 448 = 1.75 . 2^8; e2m1: 6 = 1.5 . 2^2.
// The multiplication by a power of two is exact and |x . 2^-e| <= qmax, so the conversion never saturates.  (The
// reference multiplies by an approximate reciprocal of qmax and rounds the quotient's exponent up; at amax exactly
// qmax . 2^e its hardware may give e + 1.  The compare here is exact: see fi_mi355.h.)
// A thread owns 8 consecutive elements; the 4 threads of a block are the 4 lanes of a quad.
#pragma once
#include "common.h"

#if defined(__HIPCC__)
namespace fi {

// max |v| of the lane's own 8 values
__device__ __forceinline__ float mx_amax8(const float* v) {
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
  return amax;
}

// the largest of the quad's four lane values: amax of a block of 32 from every lane's mx_amax8
__device__ __forceinline__ float mx_quad_max(float x) {
  x = fmaxf(x, lane_xor<1>(x));
  return fmaxf(x, lane_xor<2>(x));
}

// the block's scale exponent e for a format whose largest magnitude is c . 2^P, c's mantissa field MANT
template <int P, uint32_t MANT>
__device__ __forceinline__ int mx_exponent(float amax) {
  const uint32_t bits = __builtin_bit_cast(uint32_t, amax);
  const int e = (int)(bits >> 23) - 127 - P + ((bits & 0x7fffffu) > MANT ? 1 : 0);
  return min(max(e, -127), 127);
}
__device__ __forceinline__ int mx_e4m3_exponent(float amax) { return mx_exponent<8, 0x600000u>(amax); }  // 448 = 1.75 . 2^8
__device__ __forceinline__ int mx_e2m1_exponent(float amax) { return mx_exponent<2, 0x400000u>(amax); }  // 6 = 1.5 . 2^2

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
