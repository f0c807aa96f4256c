// One translation unit per (compute type, kv storage, q storage, head_dim); compiled by the Makefile with
// -DFI_PF_T16=.. -DFI_PF_KVS=.. -DFI_PF_QS=.. -DFI_PF_D=..
#include "prefill_kernel.h"

#define FI_CAT5_(a, b, c, d, e) a##b##_##c##_##d##_##e
#define FI_CAT5(a, b, c, d, e) FI_CAT5_(a, b, c, d, e)
#define FI_LAUNCHER FI_CAT5(prefill_launch_, FI_PF_T16, FI_PF_KVS, FI_PF_QS, FI_PF_D)

namespace fi {

template <bool ROPE, int GEN, int PMODE = 0, bool SINK = false>
static hipError_t launch(const PrefillKernelParams& p, hipStream_t stream) {
  auto kern = batch_prefill_kernel<FI_PF_T16, FI_PF_KVS, FI_PF_QS, FI_PF_D, ROPE, GEN, PMODE, SINK>;
  constexpr int smem = 2 * 2 * kTileKV * FI_PF_D * 2;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  const int grid = p.num_work * p.num_kv_heads;
  if (grid == 0) return hipSuccess;
  kern<<<dim3(grid), dim3(kPrefillThreads), smem, stream>>>(p);
  return hipGetLastError();
}

// feature mask of a run (prefill_kernel.h, GEN): a single feature without fused RoPE gets its own instantiation,
// combinations (and every fused-RoPE run with a feature) the all-features one
template <int PMODE>
static hipError_t launch_features(const PrefillKernelParams& p, int rope, hipStream_t stream) {
  const int gen = (p.use_alibi ? 1 : 0) | (p.logits_soft_cap > 0.f ? 2 : 0) | (p.custom_mask != nullptr ? 4 : 0) |
                  (p.prefix_len_ptr != nullptr ? 8 : 0);
#if FI_PF_QS <= 1  // 16-bit queries (enumerators are not visible to the preprocessor)
  static_assert(FI_DTYPE_F16 == 0 && FI_DTYPE_BF16 == 1, "16-bit tags");
  // attention sinks on a final output (the partial states of a split kv axis get them in their merge): the SINK
  // kernels, which exist in the plain and the all-features form
  if (p.sinks && !p.kv_tile_indices && p.num_kv_chunks <= 1) {
    if (rope) return gen ? launch<true, 15, PMODE, true>(p, stream) : launch<true, 0, PMODE, true>(p, stream);
    return gen ? launch<false, 15, PMODE, true>(p, stream) : launch<false, 0, PMODE, true>(p, stream);
  }
#else
  if (p.sinks) return hipErrorInvalidValue;  // refused on the host before it gets here
#endif
  if (rope) return gen ? launch<true, 15, PMODE>(p, stream) : launch<true, 0, PMODE>(p, stream);
  switch (gen) {
    case 0: return launch<false, 0, PMODE>(p, stream);
    case 1: return launch<false, 1, PMODE>(p, stream);
    case 2: return launch<false, 2, PMODE>(p, stream);
    case 4: return launch<false, 4, PMODE>(p, stream);
    case 8: return launch<false, 8, PMODE>(p, stream);
    default: return launch<false, 15, PMODE>(p, stream);
  }
}

hipError_t FI_LAUNCHER(const PrefillKernelParams& p, int rope, hipStream_t stream) {
#if FI_PF_T16 == 1 && FI_PF_QS == 1  // FI_DTYPE_BF16 (an enumerator: not visible to the preprocessor)
  static_assert(FI_DTYPE_BF16 == 1, "bf16 tag");
  // bf16: bf16_pv_mode picks the P.V arithmetic (fi_batch_prefill_params_t): 0 / 2 P.V on the f16 MFMA (PMODE 2),
  // 1 hi + lo bf16 halves of P (no f16 range limit on V; 25 % slower), 3 the reference's single bf16 rounding of P
  // (prefill.cuh:962-985; absolute error up to ~4e-3 on unit-variance V)
  if (p.bf16_pv_mode == 1) return launch_features<1>(p, rope, stream);
  if (p.bf16_pv_mode != 3) return launch_features<2>(p, rope, stream);
#endif
  return launch_features<0>(p, rope, stream);
}

}  // namespace fi
