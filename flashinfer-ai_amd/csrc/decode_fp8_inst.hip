// fp8-query decode instantiations (decode_fp8_kernel.h; q, K, V e4m3): output dtype (f16 | bf16) x head_dim
// (64 | 128).
#include "decode_fp8_kernel.h"

namespace fi {

hipError_t decode_fp8_launch(const DecodeKernelParams& p, int o_dtype, int head_dim, int grid, hipStream_t stream) {
  const dim3 g(grid), b(kDecodeThreads);
#define FI_CASE(T, D)                                                        \
  if (o_dtype == T && head_dim == D) {                                       \
    decode_fp8_kernel<T, D><<<g, b, 0, stream>>>(p);                         \
    return hipGetLastError();                                                \
  }
  FI_CASE(FI_DTYPE_F16, 64) FI_CASE(FI_DTYPE_F16, 128)
  FI_CASE(FI_DTYPE_BF16, 64) FI_CASE(FI_DTYPE_BF16, 128)
#undef FI_CASE
  return hipErrorInvalidValue;
}

}  // namespace fi
