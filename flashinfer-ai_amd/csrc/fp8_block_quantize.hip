// fp8 block-scale quantiser: f16 / bf16 rows -> e4m3 values with one f32 scale per row and 128 columns, the format of
// DeepSeek-V3's activations and what trtllm_fp8_block_scale_moe takes as hidden_states / hidden_states_scale
// (ref: flashinfer/fused_moe/core.py:1742-1816; the rule csrc/trtllm_fused_moe_dev_kernel.cu:141-152).
//
// Rule: fp8_block_quant.h, shared with the gated activation of moe.hip.
//
// Shape.  The quantiser's (mxfp8_quantize.hip): a row belongs to a row team (common.h), a thread owns 8 columns (one
// 16-byte load, one 8-byte store), the 16 lanes of a block share amax.  k / 8 is a multiple of 16 and the team at least
// 16 lanes, so the lanes of a block take every turn of the loop together.  The scales go out transposed, [k / 128, m],
// the reference's layout: one 4-byte store per block, m words apart.
#include "common.h"
#include "fp8_block_quant.h"

namespace fi {

constexpr int kFp8QuantThreads = 256;

struct Fp8BlockQuantArgs {
  const uint16_t* x;
  uint8_t* q;
  float* scale;
  int64_t x_stride;
  int32_t m, k, tpr_log2;
};

template <int DT>
__global__ void __launch_bounds__(kFp8QuantThreads) fp8_quantize_1x128_kernel(const Fp8BlockQuantArgs A) {
  const RowTeam team = row_team<kFp8QuantThreads>(A.tpr_log2, A.m);
  if (team.past_end) return;
  const int64_t row = team.row;
  const uint16_t* const xr = A.x + row * A.x_stride;
  for (int cc = team.lane; cc < A.k / 8; cc += team.size) {
    const int col = cc * 8;
    float v[8];
    load_16bit<DT, 8>(xr + col, v);
    u32x2 q;
    const float s = fp8_block_quantize8(v, q);
    *(u32x2*)(A.q + row * A.k + col) = q;
    if ((cc & (kFp8BlockLanes - 1)) == 0) A.scale[(int64_t)(cc / kFp8BlockLanes) * A.m + row] = s;
  }
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_fp8_quantize_1x128(const fi_fp8_quantize_1x128_params_t* p, fi_stream_t stream) {
  FI_REQUIRE(p, "fp8_quantize_1x128: null params");
  FI_REQUIRE(p->m >= 0 && p->k >= 0, "fp8_quantize_1x128: negative size (m %d, k %d)", p->m, p->k);
  FI_REQUIRE(p->k % kFp8Block == 0, "fp8_quantize_1x128: k %d must be a multiple of 128", p->k);
  FI_REQUIRE(p->dtype == FI_DTYPE_F16 || p->dtype == FI_DTYPE_BF16, "fp8_quantize_1x128: dtype %d is not f16 or bf16", p->dtype);
  if (p->m == 0 || p->k == 0) return 0;
  FI_REQUIRE(p->input && p->q && p->scale, "fp8_quantize_1x128: null tensor");
  FI_REQUIRE(p->input_stride >= p->k, "fp8_quantize_1x128: input stride %lld is smaller than k %d", (long long)p->input_stride,
             p->k);
  FI_REQUIRE(((uintptr_t)p->input % 16) == 0 && p->input_stride % 8 == 0 && ((uintptr_t)p->q % 8) == 0 &&
                 ((uintptr_t)p->scale % 4) == 0,
             "fp8_quantize_1x128: input must be 16-byte aligned with a row stride that is a multiple of 8, q 8-byte and "
             "scale 4-byte aligned");
  Fp8BlockQuantArgs a{};
  a.x = (const uint16_t*)p->input;
  a.q = (uint8_t*)p->q;
  a.scale = p->scale;
  a.x_stride = p->input_stride;
  a.m = p->m;
  a.k = p->k;
  a.tpr_log2 = row_team_log2(p->k / 8, kFp8QuantThreads);  // k / 8 >= 16: a team holds whole blocks
  const uint32_t grid = (uint32_t)ceil_div<int64_t>(p->m, kFp8QuantThreads >> a.tpr_log2);
  if (p->dtype == FI_DTYPE_F16)
    fp8_quantize_1x128_kernel<FI_DTYPE_F16><<<dim3(grid), dim3(kFp8QuantThreads), 0, (hipStream_t)stream>>>(a);
  else
    fp8_quantize_1x128_kernel<FI_DTYPE_BF16><<<dim3(grid), dim3(kFp8QuantThreads), 0, (hipStream_t)stream>>>(a);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}
