// RMSNorm (plain and Gemma, row form and head form) and fused add + RMSNorm.
// ref: include/flashinfer/norm.cuh (RMSNormKernel :29-140, QKRMSNormKernel :142-260, FusedAddRMSNormKernel :264-355),
// csrc/norm.cu:24-162, flashinfer/norm.py.
//
// Shape.  One kernel template serves every form.  A row of `hidden` 16-bit elements is owned by one workgroup
// (row form, 64 ... 1024 threads chosen from hidden) or by one wave (head form, four rows per workgroup).  Each
// thread converts its elements to f32, sums their squares, the sum is reduced over the 64 lanes by cross-lane moves
// and over the waves through LDS in index order, and the thread scales what it holds and stores it.  A thread writes
// exactly the elements it read, so `out` may be `in`.
//
//   vector path   16-byte loads and stores (8 elements); a thread keeps its K <= 8 chunks of the row as f32 in
//                 registers between the sum and the scale, so the row is read once.  Up to K = 4 the weight chunks
//                 are fetched with the row and wait in registers too (they come from L2 after the first workgroup).
//                 Needs hidden % 8 == 0 and 16-byte aligned bases and strides; K * threads * 8 >= hidden.
//   scalar path   any hidden, stride and alignment (hidden = 111, 500, a view at an odd offset): 2-byte accesses
//                 and the row is read a second time for the scale.  A row is at most 128 KB (256 KB with the
//                 residual), so the second read is served by L2 and HBM still sees it once.
//
// Fused add: s = f32(input) + f32(residual) is formed once; residual gets T(s), while the sum of squares and the
// output use the unrounded s (norm.cuh:297-302, 345).  The scalar path forms s again in its second pass from the
// still-unwritten input and residual, which gives the same bits.
#include <algorithm>

#include "common.h"

namespace fi {

constexpr int kNormMaxThreads = 1024;
constexpr int kNormHeadRows = 4;         // head form: waves (rows) per workgroup
constexpr int kNormTargetChunks = 4;     // row form: 16-byte chunks per thread the thread count is chosen for
constexpr int kNormMaxChunks = 8;        // K of the largest instance: 1024 threads * 8 chunks * 8 = 65536 elements
constexpr int kNormHeadScalarMax = 1024; // head form, scalar path: longer rows go to the row form

struct NormArgs {
  const uint16_t* x;  // plain: in;  fused add: input (in/out)
  uint16_t* y;        // plain: out; fused add: residual (in/out)
  const uint16_t* weight;
  int64_t x_stride_n, x_stride_h, y_stride_n, y_stride_h;
  uint32_t num_rows, num_heads;
  int32_t hidden;
  float eps, weight_bias, rcp_hidden;
};

// sum over the row's threads: the wave (WAVE) or the workgroup; every thread gets the total
template <bool WAVE>
__device__ __forceinline__ float row_sum(float v, float* wave_tot) {
  v = group_sum<64>(v);
  if constexpr (WAVE) return v;
  const int num_waves = blockDim.x >> 6;
  if (num_waves == 1) return v;
  if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
  for (int w = 0; w < num_waves; ++w) t += wave_tot[w];
  return t;
}

// K > 0: vector path with K chunks per thread in registers.  K == 0: scalar path (VEC == 1).
template <int DT, bool ADD, int K, bool WAVE>
__global__ void __launch_bounds__(WAVE ? 64 * kNormHeadRows : kNormMaxThreads) rmsnorm_kernel(NormArgs A) {
  __shared__ float wave_tot[kNormMaxThreads / 64];
  const int tid = WAVE ? (threadIdx.x & 63) : threadIdx.x;
  const int nthr = WAVE ? 64 : blockDim.x;
  const uint32_t row = WAVE ? blockIdx.x * kNormHeadRows + (threadIdx.x >> 6) : blockIdx.x;
  if (WAVE && row >= A.num_rows) return;  // whole waves leave; the head form has no workgroup barrier
  const uint32_t tok = A.num_heads == 1 ? row : row / A.num_heads;
  const uint32_t head = row - tok * A.num_heads;
  const uint16_t* x = A.x + (int64_t)tok * A.x_stride_n + (int64_t)head * A.x_stride_h;
  uint16_t* y = A.y + (int64_t)tok * A.y_stride_n + (int64_t)head * A.y_stride_h;
  uint16_t* dst = ADD ? const_cast<uint16_t*>(x) : y;
  float sum = 0.f;

  if constexpr (K > 0) {
    const int nc = A.hidden >> 3;
    float s[K][8];
    // the weight chunks are fetched with the row and stay packed until they are used; the 8-chunk instance has no
    // registers left for that and fetches them after the sum
    constexpr bool kWeightAhead = K <= 4;
    u32x4 w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int c = tid + k * nthr;
#pragma unroll
      for (int j = 0; j < 8; ++j) s[k][j] = 0.f;
      if (c < nc) {
        load_16bit<DT, 8>(x + c * 8, s[k]);
        if constexpr (kWeightAhead) w[k] = *(const u32x4*)(A.weight + c * 8);
        if constexpr (ADD) {
          float r[8];
          load_16bit<DT, 8>(y + c * 8, r);
#pragma unroll
          for (int j = 0; j < 8; ++j) r[j] = s[k][j] = s[k][j] + r[j];
          store_16bit<DT, 8>(y + c * 8, r);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += s[k][j] * s[k][j];
    const float scale = rsqrtf(row_sum<WAVE>(sum, wave_tot) * A.rcp_hidden + A.eps);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int c = tid + k * nthr;
      if (c < nc) {
        float wf[8];
        if constexpr (!kWeightAhead) w[k] = *(const u32x4*)(A.weight + c * 8);
        KVTraits<DT>::unpack(w[k], wf);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[k][j] = s[k][j] * scale * (A.weight_bias + wf[j]);
        store_16bit<DT, 8>(dst + c * 8, s[k]);
      }
    }
  } else {
    auto element = [&](int i) {
      float s = load_f16_or_bf16(x, i, DT);
      if constexpr (ADD) s += load_f16_or_bf16(y, i, DT);
      return s;
    };
    for (int i = tid; i < A.hidden; i += nthr) {
      const float s = element(i);
      sum += s * s;
    }
    const float scale = rsqrtf(row_sum<WAVE>(sum, wave_tot) * A.rcp_hidden + A.eps);
    for (int i = tid; i < A.hidden; i += nthr) {
      const float s = element(i);
      if constexpr (ADD) y[i] = f32_to_16bit(s, DT);
      dst[i] = f32_to_16bit(s * scale * (A.weight_bias + load_f16_or_bf16(A.weight, i, DT)), DT);
    }
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int DT, bool ADD, int K, bool WAVE>
static void launch_instance(const NormArgs& a, int threads, hipStream_t stream) {
  const uint32_t grid = WAVE ? ceil_div<uint32_t>(a.num_rows, kNormHeadRows) : a.num_rows;
  rmsnorm_kernel<DT, ADD, K, WAVE><<<dim3(grid), dim3(WAVE ? 64 * kNormHeadRows : threads), 0, stream>>>(a);
}

// smallest instantiated K (1, 2, 4, 8) that is >= need
template <int DT, bool ADD, bool WAVE>
static void launch_vector(const NormArgs& a, int need, int threads, hipStream_t stream) {
  if (need <= 1) launch_instance<DT, ADD, 1, WAVE>(a, threads, stream);
  else if (need <= 2) launch_instance<DT, ADD, 2, WAVE>(a, threads, stream);
  else if (need <= 4) launch_instance<DT, ADD, 4, WAVE>(a, threads, stream);
  else launch_instance<DT, ADD, 8, WAVE>(a, threads, stream);
}

// The host's choice of path: vector when every access can be 16 bytes, the wave-per-row form for head-form rows a
// wave can hold, otherwise one workgroup per row.
template <int DT, bool ADD>
static int launch_norm(const NormArgs& a, hipStream_t stream) {
  const bool heads = a.num_heads > 1;
  const bool vec = a.hidden % 8 == 0 && aligned16(a.x) && aligned16(a.y) && aligned16(a.weight) &&
                   a.x_stride_n % 8 == 0 && a.y_stride_n % 8 == 0 &&
                   (!heads || (a.x_stride_h % 8 == 0 && a.y_stride_h % 8 == 0));
  const int nc = a.hidden / 8;
  if constexpr (!ADD) {
    if (heads && vec && nc <= 64 * kNormMaxChunks) {
      launch_vector<DT, false, true>(a, ceil_div(nc, 64), 0, stream);
      return 0;
    }
    if (heads && !vec && a.hidden <= kNormHeadScalarMax) {
      launch_instance<DT, false, 0, true>(a, 0, stream);
      return 0;
    }
  }
  if (vec) {
    const int threads = std::min(kNormMaxThreads, ceil_div(ceil_div(nc, kNormTargetChunks), 64) * 64);
    launch_vector<DT, ADD, false>(a, ceil_div(nc, threads), threads, stream);
  } else {
    launch_instance<DT, ADD, 0, false>(a, std::min(kNormMaxThreads, ceil_div(a.hidden, 64) * 64), stream);
  }
  return 0;
}

static int check_common(const char* what, int32_t batch, int32_t num_heads, int32_t hidden, int32_t dtype) {
  FI_REQUIRE(batch >= 0, "%s: negative batch %d", what, batch);
  FI_REQUIRE(hidden >= 1 && hidden <= FI_NORM_MAX_HIDDEN, "%s: hidden %d out of range [1, %d]", what, hidden,
             FI_NORM_MAX_HIDDEN);
  FI_REQUIRE(num_heads >= 1, "%s: num_heads %d must be positive", what, num_heads);
  FI_REQUIRE(dtype == FI_DTYPE_F16 || dtype == FI_DTYPE_BF16, "%s: dtype %d is not f16 or bf16", what, dtype);
  FI_REQUIRE((int64_t)batch * num_heads <= INT32_MAX, "%s: batch %d x num_heads %d exceeds 2^31 - 1 rows", what, batch,
             num_heads);
  return 0;
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_rmsnorm(const fi_rmsnorm_params_t* p, fi_stream_t stream) {
  FI_REQUIRE(p, "rmsnorm: null params");
  if (int rc = check_common("rmsnorm", p->batch, p->num_heads, p->hidden, p->dtype)) return rc;
  if (p->batch == 0) return 0;
  FI_REQUIRE(p->in && p->weight && p->out, "rmsnorm: null tensor");
  const bool heads = p->num_heads > 1;
  FI_REQUIRE(p->in_stride_n >= p->hidden && p->out_stride_n >= p->hidden &&
                 (!heads || (p->in_stride_h >= p->hidden && p->out_stride_h >= p->hidden)),
             "rmsnorm: a stride is smaller than hidden %d", p->hidden);
  NormArgs a{};
  a.x = (const uint16_t*)p->in;
  a.y = (uint16_t*)p->out;
  a.weight = (const uint16_t*)p->weight;
  a.x_stride_n = p->in_stride_n;
  a.y_stride_n = p->out_stride_n;
  a.x_stride_h = heads ? p->in_stride_h : 0;
  a.y_stride_h = heads ? p->out_stride_h : 0;
  a.num_rows = (uint32_t)p->batch * (uint32_t)p->num_heads;
  a.num_heads = (uint32_t)p->num_heads;
  a.hidden = p->hidden;
  a.eps = p->eps;
  a.weight_bias = p->weight_bias;
  a.rcp_hidden = 1.f / (float)p->hidden;
  if (p->dtype == FI_DTYPE_F16)
    launch_norm<FI_DTYPE_F16, false>(a, (hipStream_t)stream);
  else
    launch_norm<FI_DTYPE_BF16, false>(a, (hipStream_t)stream);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}

extern "C" FI_API int fi_fused_add_rmsnorm(const fi_fused_add_rmsnorm_params_t* p, fi_stream_t stream) {
  FI_REQUIRE(p, "fused_add_rmsnorm: null params");
  if (int rc = check_common("fused_add_rmsnorm", p->batch, 1, p->hidden, p->dtype)) return rc;
  if (p->batch == 0) return 0;
  FI_REQUIRE(p->input && p->residual && p->weight, "fused_add_rmsnorm: null tensor");
  FI_REQUIRE(p->input_stride >= p->hidden && p->residual_stride >= p->hidden,
             "fused_add_rmsnorm: a stride is smaller than hidden %d", p->hidden);
  NormArgs a{};
  a.x = (const uint16_t*)p->input;
  a.y = (uint16_t*)p->residual;
  a.weight = (const uint16_t*)p->weight;
  a.x_stride_n = p->input_stride;
  a.y_stride_n = p->residual_stride;
  a.num_rows = (uint32_t)p->batch;
  a.num_heads = 1;
  a.hidden = p->hidden;
  a.eps = p->eps;
  a.weight_bias = p->weight_bias;
  a.rcp_hidden = 1.f / (float)p->hidden;
  if (p->dtype == FI_DTYPE_F16)
    launch_norm<FI_DTYPE_F16, true>(a, (hipStream_t)stream);
  else
    launch_norm<FI_DTYPE_BF16, true>(a, (hipStream_t)stream);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}
