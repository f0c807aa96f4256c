// 16x16x32 matrix-core decode, MULTI form (several query tokens per request; decode_mfma16_kernel.h): q dtype
// (f16 | bf16) x cache dtype (same | e4m3 | e5m2) x head_dim (64 | 128), paged, no fused RoPE.
#include "decode_mfma16_kernel.h"

namespace fi {

hipError_t decode_mfma16_multi_launch(const DecodeMultiParams& p, int q_dtype, int kv_dtype, int head_dim, int grid,
                                      hipStream_t stream) {
#define FI_CASE(T, K, D)                                                                              \
  if (q_dtype == T && kv_dtype == K && head_dim == D) {                                               \
    decode_mfma16_kernel<T, K, D, true, false, false, true><<<dim3(grid), dim3(kDecodeThreads), 0, stream>>>(p); \
    return hipGetLastError();                                                                         \
  }
#define FI_ROW(T, K) FI_CASE(T, K, 64) FI_CASE(T, K, 128)
  FI_ROW(FI_DTYPE_F16, FI_DTYPE_F16)
  FI_ROW(FI_DTYPE_F16, FI_DTYPE_FP8_E4M3)
  FI_ROW(FI_DTYPE_F16, FI_DTYPE_FP8_E5M2)
  FI_ROW(FI_DTYPE_BF16, FI_DTYPE_BF16)
  FI_ROW(FI_DTYPE_BF16, FI_DTYPE_FP8_E4M3)
  FI_ROW(FI_DTYPE_BF16, FI_DTYPE_FP8_E5M2)
#undef FI_ROW
#undef FI_CASE
  return hipErrorInvalidValue;
}

}  // namespace fi
