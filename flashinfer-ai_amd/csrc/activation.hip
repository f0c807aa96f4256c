// Gated activations of the MLP: out[t, j] = act(in[t, j]) * in[t, d + j] for silu, gelu (erf) and gelu_tanh.
// ref: flashinfer/activation.py:33-88 (the three formulas), include/flashinfer/activation.cuh (act_and_mul_kernel).
//
// Shape.  A thread owns one chunk of VEC output elements of a token: it loads the gate chunk and the up chunk
// (two loads of VEC * 2 bytes), does the arithmetic in f32 and stores one chunk.  grid.x covers the chunks of a
// row, grid.y the tokens (a thread walks tokens in steps of grid.y only beyond 65535 tokens).  Workgroups are 64
// threads while the whole problem is small, so that one token (decode) still spreads over many compute units, and
// 256 threads otherwise.  VEC is 8 (16-byte accesses) when d % 8 == 0 and both bases are 16-byte aligned, 4 when
// d % 4 == 0 (what the Python layer's 16-byte rule on the 2 d wide input guarantees), else 1.
#include <algorithm>

#include "common.h"

namespace fi {

constexpr int kActMaxGridY = 65535;
constexpr int kActSmallProblem = 1 << 16;  // chunks below which workgroups are one wave

template <int ACT>
__device__ __forceinline__ float activation(float x) {
  if constexpr (ACT == FI_ACT_SILU) {
    return x * fast_rcp(1.f + __expf(-x));
  } else if constexpr (ACT == FI_ACT_GELU) {
    return x * 0.5f * (1.f + erff(x * 0.70710678118654752440f));
  } else {
    // 0.5 (1 + tanh u) = 1 / (1 + exp(-2 u)): the same function without the cancellation at very negative u
    const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
    return x * fast_rcp(1.f + __expf(-2.f * u));
  }
}

template <int DT, int ACT, int VEC>
__global__ void __launch_bounds__(256) act_and_mul_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out,
                                                          int64_t tokens, int d) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= d / VEC) return;
  for (int64_t t = blockIdx.y; t < tokens; t += gridDim.y) {
    const uint16_t* row = in + t * 2 * d + c * VEC;
    float g[VEC], u[VEC];
    load_16bit<DT, VEC>(row, g);
    load_16bit<DT, VEC>(row + d, u);
#pragma unroll
    for (int j = 0; j < VEC; ++j) g[j] = activation<ACT>(g[j]) * u[j];
    store_16bit<DT, VEC>(out + t * d + c * VEC, g);
  }
}

template <int DT, int ACT, int VEC>
static void launch_act_vec(const fi_act_and_mul_params_t& p, hipStream_t stream) {
  const int chunks = p.d / VEC;
  const int threads = (int64_t)chunks * p.tokens < kActSmallProblem ? 64 : 256;
  const dim3 grid(ceil_div(chunks, threads), (unsigned)std::min<int64_t>(p.tokens, kActMaxGridY));
  act_and_mul_kernel<DT, ACT, VEC><<<grid, dim3(threads), 0, stream>>>((const uint16_t*)p.in, (uint16_t*)p.out,
                                                                      p.tokens, p.d);
}

template <int DT, int ACT>
static void launch_act(const fi_act_and_mul_params_t& p, hipStream_t stream) {
  const uintptr_t bases = (uintptr_t)p.in | (uintptr_t)p.out;
  if (p.d % 8 == 0 && bases % 16 == 0) launch_act_vec<DT, ACT, 8>(p, stream);
  else if (p.d % 4 == 0 && bases % 8 == 0) launch_act_vec<DT, ACT, 4>(p, stream);
  else launch_act_vec<DT, ACT, 1>(p, stream);
}

template <int DT>
static void launch_act_dtype(const fi_act_and_mul_params_t& p, hipStream_t stream) {
  if (p.act == FI_ACT_SILU) launch_act<DT, FI_ACT_SILU>(p, stream);
  else if (p.act == FI_ACT_GELU) launch_act<DT, FI_ACT_GELU>(p, stream);
  else launch_act<DT, FI_ACT_GELU_TANH>(p, stream);
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_act_and_mul(const fi_act_and_mul_params_t* p, fi_stream_t stream) {
  FI_REQUIRE(p, "act_and_mul: null params");
  FI_REQUIRE(p->tokens >= 0, "act_and_mul: negative tokens %lld", (long long)p->tokens);
  FI_REQUIRE(p->d >= 1 && p->d <= FI_NORM_MAX_HIDDEN, "act_and_mul: hidden d %d out of range [1, %d]", p->d,
             FI_NORM_MAX_HIDDEN);
  FI_REQUIRE(p->dtype == FI_DTYPE_F16 || p->dtype == FI_DTYPE_BF16, "act_and_mul: dtype %d is not f16 or bf16",
             p->dtype);
  FI_REQUIRE(p->act == FI_ACT_SILU || p->act == FI_ACT_GELU || p->act == FI_ACT_GELU_TANH,
             "act_and_mul: unknown activation code %d", p->act);
  if (p->tokens == 0) return 0;
  FI_REQUIRE(p->in && p->out, "act_and_mul: null tensor");
  if (p->dtype == FI_DTYPE_F16)
    launch_act_dtype<FI_DTYPE_F16>(*p, (hipStream_t)stream);
  else
    launch_act_dtype<FI_DTYPE_BF16>(*p, (hipStream_t)stream);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}
