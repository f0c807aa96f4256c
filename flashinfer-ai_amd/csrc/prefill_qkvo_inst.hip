// Instantiations of prefill_qkvo_kernel (head_dim_qk 192 / head_dim_vo 128): f16, and bf16 in its three P.V modes.
#include "prefill_qkvo_kernel.h"

namespace fi {

template <int T16, int PMODE>
static hipError_t launch_qkvo(const PrefillQkvoParams& p, hipStream_t stream) {
  auto kern = prefill_qkvo_kernel<T16, PMODE>;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kQkvoSmemBytes);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  const int grid = p.num_work * p.num_kv_heads;
  if (grid == 0) return hipSuccess;
  kern<<<dim3(grid), dim3(kPrefillThreads), kQkvoSmemBytes, stream>>>(p);
  return hipGetLastError();
}

// dtype: FI_DTYPE_F16 / FI_DTYPE_BF16 (q, k, v and o); pmode: the bf16 P.V mode (0 single bf16 P, 1 hi + lo, 2 f16 P.V)
hipError_t prefill_qkvo_launch(const PrefillQkvoParams& p, int dtype, int pmode, hipStream_t stream) {
  if (dtype == FI_DTYPE_F16) return launch_qkvo<FI_DTYPE_F16, 0>(p, stream);
  if (pmode == 2) return launch_qkvo<FI_DTYPE_BF16, 2>(p, stream);
  if (pmode == 1) return launch_qkvo<FI_DTYPE_BF16, 1>(p, stream);
  return launch_qkvo<FI_DTYPE_BF16, 0>(p, stream);
}

}  // namespace fi
