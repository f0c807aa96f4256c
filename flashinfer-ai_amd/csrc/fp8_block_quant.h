// The fp8 block-scale quantisation rule (DeepSeek's "1 x 128" activations) as device code: what the gated activation of
// the fp8 block-scale MoE layer (moe.hip) and the quantiser fi_fp8_quantize_1x128 (fp8_block_quantize.hip) share, so that
// both produce the same f32 scale and the same e4m3 bytes for the same f32 values.  The sibling of mx_quant.h, whose
// scales are powers of two per 32 elements; here a scale is any positive normal f32 per 128 elements.
//
// Per row and block of 128 columns: amax = max |x|; s = max(amax / 448, 2^-126); q = e4m3(clamp(x / s, -448, 448)),
// round to nearest even.  amax / 448 is the reference kernel's rule (csrc/trtllm_fused_moe_dev_kernel.cu:141-152).  The
// floor keeps s a normal f32 and turns an all-zero block into q = 0 instead of 0 / 0.  Both divisions are IEEE
// divisions (the library is built without fast-math), so s is the correctly rounded quotient; x / s may then land one ulp
// above 448, and byte 0x7F is NaN in e4m3fn: hence the clamp.
// A thread owns 8 consecutive elements; the 16 threads of a block are 16 consecutive, 16-aligned lanes (one DPP row).
#pragma once
#include "common.h"
#include "mx_quant.h"  // mx_amax8

#if defined(__HIPCC__)
namespace fi {

constexpr int kFp8Block = 128;          // columns per scale
constexpr int kFp8BlockLanes = 128 / 8;  // lanes per block, 8 columns each

// the block's scale from its amax: the largest of the 16 lanes' own maxima (every lane of the block calls it)
__device__ __forceinline__ float fp8_block_scale(float lane_amax) {
  return fmaxf(group_reduce<kFp8BlockLanes, RedMax>(lane_amax) / 448.0f, 0x1p-126f);
}

// The clamped conversion: 4 f32 as 4 fp8 bytes of type DT (e4m3: largest finite 448, e5m2: 57344), round to nearest
// even, saturating -- a value beyond the largest finite one would become NaN (e4m3fn) or infinity (e5m2).  Shared with
// the MLA rope-and-quantise kernel (rope.hip).
template <int DT = FI_DTYPE_FP8_E4M3>
__device__ __forceinline__ uint32_t fp8_pack4_saturating(float y0, float y1, float y2, float y3) {
  constexpr float kMax = DT == FI_DTYPE_FP8_E4M3 ? 448.f : 57344.f;
  y0 = __builtin_amdgcn_fmed3f(y0, -kMax, kMax);
  y1 = __builtin_amdgcn_fmed3f(y1, -kMax, kMax);
  y2 = __builtin_amdgcn_fmed3f(y2, -kMax, kMax);
  y3 = __builtin_amdgcn_fmed3f(y3, -kMax, kMax);
  int packed;
  if constexpr (DT == FI_DTYPE_FP8_E4M3) {
    packed = __builtin_amdgcn_cvt_pk_fp8_f32(y0, y1, 0, false);
    packed = __builtin_amdgcn_cvt_pk_fp8_f32(y2, y3, packed, true);
  } else {
    packed = __builtin_amdgcn_cvt_pk_bf8_f32(y0, y1, 0, false);
    packed = __builtin_amdgcn_cvt_pk_bf8_f32(y2, y3, packed, true);
  }
  return (uint32_t)packed;
}

// 8 values divided by the block's scale as 8 e4m3 bytes
__device__ __forceinline__ u32x2 fp8_block_pack8(const float* v, float s) {
  uint32_t w[2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
    w[h] = fp8_pack4_saturating(v[4 * h] / s, v[4 * h + 1] / s, v[4 * h + 2] / s, v[4 * h + 3] / s);
  return u32x2{w[0], w[1]};
}

// The whole rule for a lane's 8 values of a block (amax of 128 -> s -> pack): returns s, the bytes go to `q`.
__device__ __forceinline__ float fp8_block_quantize8(const float* v, u32x2& q) {
  const float s = fp8_block_scale(mx_amax8(v));
  q = fp8_block_pack8(v, s);
  return s;
}

}  // namespace fi
#endif  // __HIPCC__
