// Shared host/device helpers for libfi_mi355.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <optional>

#include "fi_mi355.h"

namespace fi {

// ---- host-side error channel (ref: include/flashinfer/exception.h:23, 74-87) ----
int set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
const char* last_error();

#define FI_REQUIRE(cond, ...)                 \
  do {                                        \
    if (!(cond)) return ::fi::set_error(__VA_ARGS__); \
  } while (0)

#define FI_HIP_CALL(expr)                                                                 \
  do {                                                                                    \
    hipError_t e__ = (expr);                                                              \
    if (e__ != hipSuccess)                                                                \
      return ::fi::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, \
                             __LINE__);                                                   \
  } while (0)

// ---- kernel-choice switches (lib.hip): the FI_* variables of INTEGRATION.md ----
// Each starts as the environment gave it when the library was loaded; fi_set_option changes it in the running process.
enum Option {
  OPT_NUM_CUS,
  OPT_DECODE_MFMA16,
  OPT_GEMM_WS_MIN_TILES,
  OPT_GEMM_DMA_TM,
  OPT_GEMM_BIG,
  OPT_GEMM_BIG_MIN_TILES,
  OPT_GEMM_BIG_FOLD_MIN_TILES,
  OPT_GEMM_HW_SCALES,
  OPT_MM_FP4_KERNEL,
  OPT_COUNT
};
// The switch's value; none when neither fi_set_option nor the environment gave it one.  One atomic load: a call
// that must not see a switch change under it reads each switch once, at its top.
std::optional<int> option(Option o);

inline size_t dtype_size(int dt) {
  switch (dt) {
    case FI_DTYPE_F16:
    case FI_DTYPE_BF16:
      return 2;
    case FI_DTYPE_FP8_E4M3:
    case FI_DTYPE_FP8_E5M2:
      return 1;
    case FI_DTYPE_F32:
      return 4;
    default:
      return 0;
  }
}

template <typename T>
inline T ceil_div(T a, T b) {
  return (a + b - 1) / b;
}

// A row team: the threads of a workgroup that share one row of a row-indexed kernel (mxfp8_quantize.hip; gather, gated
// activation and finalize of moe.hip) -- a power of two of them from one quad to the workgroup, enough for the row's
// chunks when it can be (this is its log2); more chunks take further passes.  row_team() below is the device side.
inline int row_team_log2(int64_t chunks, int threads) {
  int l = 2;
  while ((1 << l) < threads && (1ll << l) < chunks) ++l;
  return l;
}

// 16-byte aligned bump allocator over a caller-owned workspace; returns byte offsets.
// ref: AlignedAllocator, include/flashinfer/allocator.h:32-59.
struct OffsetAllocator {
  size_t cap;
  size_t used = 0;
  bool ok = true;
  explicit OffsetAllocator(size_t capacity) : cap(capacity) {}
  int64_t alloc(size_t bytes, size_t align = 16) {
    size_t start = (used + align - 1) / align * align;
    if (start + bytes > cap) {
      ok = false;
      return 0;
    }
    used = start + bytes;
    return (int64_t)start;
  }
};

// The planners' chunk search: the smallest value in [lo, hi] for which too_many(value) is false (hi if it never is,
// lo if the range is empty).  too_many must not turn true again as the value grows.  The host planners search in
// int64_t whatever their bounds' types; the planners on the device (plan_device.h) name a 32-bit T.
template <typename T>
struct search_bound {
  using type = T;  // keeps lo and hi out of the deduction of T
};
template <typename T = int64_t, class Pred>
__host__ __device__ inline T smallest_fitting(typename search_bound<T>::type lo, typename search_bound<T>::type hi,
                                              Pred too_many) {
  while (lo < hi) {
    const T mid = (lo + hi) / 2;
    if (too_many(mid)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Division by a runtime-constant 32-bit divisor using a precomputed multiplier (round-up method,
// Granlund & Montgomery 1994): q = (umulhi(n, m) + n) >> l, valid for n < 2^31.
struct FastDiv {
  uint32_t d, m, l;
  FastDiv() : d(1), m(0), l(0) {}
  explicit FastDiv(uint32_t divisor) : d(divisor) {
    l = 0;
    while ((1ull << l) < d) ++l;
    m = (uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
  }
};

}  // namespace fi

#if defined(__HIPCC__)
namespace fi {

using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;

__device__ __forceinline__ uint32_t fast_div(uint32_t n, const FastDiv& fd) {
  return (__umulhi(n, fd.m) + n) >> fd.l;
}

struct RowTeam {
  int lane, size;  // this thread in its team; threads per team (row_team_log2)
  int64_t row;
  bool past_end;   // row >= rows.  Whole quads leave: the size is a multiple of 4
};
template <int THREADS>
__device__ __forceinline__ RowTeam row_team(int size_log2, int32_t rows) {
  const int size = 1 << size_log2;
  const int64_t row = (int64_t)blockIdx.x * (THREADS >> size_log2) + (threadIdx.x >> size_log2);
  return RowTeam{(int)(threadIdx.x & (size - 1)), size, row, row >= rows};
}

constexpr float kLog2e = 1.44269504088896340736f;

// accurate sin/cos kept out of line: only used to seed rotations / in the fused-RoPE variants
__device__ __attribute__((noinline)) static void sincos_ool(float x, float* sn, float* cs) {
  sincosf(x, sn, cs);
}

// sin / cos of an angle in radians: x = k * 2pi + y with |y| <= pi (two-term Cody-Waite reduction), then
// the hardware v_sin / v_cos on y / 2pi.  Absolute error ~1e-6 for |x| up to ~1e5 (RoPE angles).
__device__ __forceinline__ void fast_sincos(float x, float* sn, float* cs) {
  const float k = rintf(x * 0.15915494309189535f);
  float y = __builtin_fmaf(-k, 6.2831854820251465f, x);       // 2pi high part (float)
  y = __builtin_fmaf(-k, -1.7484555e-07f, y);                 // 2pi - float(2pi)
  const float rev = y * 0.15915494309189535f;
  *sn = __builtin_amdgcn_sinf(rev);
  *cs = __builtin_amdgcn_cosf(rev);
}

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float fast_log2(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
// tanh(x) = 1 - 2 / (2^(2 x log2e) + 1)   (ref uses tanh.approx: include/flashinfer/math.cuh:120-150)
__device__ __forceinline__ float fast_tanh(float x) {
  float e = fast_exp2(x * 2.885390081777927f);
  return 1.0f - 2.0f * fast_rcp(e + 1.0f);
}

// Attention sink (ref: AttentionSink, flashinfer/jit/attention/variants.py:17-53): one more term 2^sink_log2 in the
// softmax denominator of a row, without a value vector.  Given the row's final running state (m, l) in base 2 --
// the accumulators hold sum_j 2^(s_j - m) v_j, l = sum_j 2^(s_j - m) -- this returns what the finalize block of a
// kernel multiplies the accumulators by and the row's lse, i.e. the state merged with (0, sink_log2):
//   m' = max(m, sink_log2), sa = 2^(m - m'), l' = l sa + 2^(sink_log2 - m');  inv = sa / l', lse = m' + log2(l').
// m must be finite (the kernels start it at -1e30).  sink_log2 = -inf gives sa = 1 and l' = l exactly: inv and lse
// are then bit for bit the values without a sink; an empty row (l = 0) with it gives inv = 0, lse = FI_NEG_INF.
// A state that carries a power-of-two factor 2^k in l (and in its accumulators) passes sink_log2 + k.
__device__ __forceinline__ void fold_sink(float m, float l, float sink_log2, float& inv, float& lse) {
  const float m2 = fmaxf(m, sink_log2);
  const float sa = fast_exp2(m - m2);
  const float l2 = __builtin_fmaf(l, sa, fast_exp2(sink_log2 - m2));
  const bool empty = !(l2 > 0.f);
  inv = empty ? 0.f : sa * (1.0f / l2);
  lse = empty ? FI_NEG_INF : m2 + fast_log2(l2);
}

// ---- cross-lane moves ----
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}
constexpr int DPP_QUAD_XOR1 = 0xB1;   // quad_perm:[1,0,3,2]
constexpr int DPP_QUAD_XOR2 = 0x4E;   // quad_perm:[2,3,0,1]
constexpr int DPP_ROW_HALF_MIRROR = 0x141;
constexpr int DPP_ROW_MIRROR = 0x140;
constexpr int DPP_ROW_ROR8 = 0x128;

// value of lane (lane ^ MASK)
template <int MASK>
__device__ __forceinline__ float lane_xor(float x) {
  if constexpr (MASK == 1)
    return dpp_mov<DPP_QUAD_XOR1>(x);
  else if constexpr (MASK == 2)
    return dpp_mov<DPP_QUAD_XOR2>(x);
  else if constexpr (MASK == 8)
    return dpp_mov<DPP_ROW_ROR8>(x);
  else
    return __shfl_xor(x, MASK, 64);
}

// Sum over groups of N consecutive lanes (N a power of two, groups aligned); every lane of the group
// receives the total.  Steps inside a 16-lane row are DPP adds (no LDS traffic).
template <int N>
__device__ __forceinline__ float group_sum(float x) {
  if constexpr (N >= 2) x += dpp_mov<DPP_QUAD_XOR1>(x);
  if constexpr (N >= 4) x += dpp_mov<DPP_QUAD_XOR2>(x);
  if constexpr (N >= 8) x += dpp_mov<DPP_ROW_HALF_MIRROR>(x);
  if constexpr (N >= 16) x += dpp_mov<DPP_ROW_MIRROR>(x);
  if constexpr (N >= 32) x += __shfl_xor(x, 16, 64);
  if constexpr (N >= 64) x += __shfl_xor(x, 32, 64);
  return x;
}

// ---- scans and reductions over a wave and over a workgroup ----
// Only exact operations reduce here: maxima, and sums of integers.  A float sum over lanes has its bits fixed by its
// order and stays with its kernel (group_sum above, the ladders of merge.hip, moe.hip and norm.hip); the one float sum
// here is the scan, whose order is part of its definition.
struct RedMax {
  static __device__ __forceinline__ float of(float a, float b) { return fmaxf(a, b); }
  static __device__ __forceinline__ uint32_t of(uint32_t a, uint32_t b) { return max(a, b); }
};
struct RedSum {
  static __device__ __forceinline__ uint32_t of(uint32_t a, uint32_t b) { return a + b; }
  static __device__ __forceinline__ int of(int a, int b) { return a + b; }
};

// OP over the 64 lanes, the result in every lane
template <class OP, typename T>
__device__ __forceinline__ T wave_reduce(T v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = OP::of(v, __shfl_xor(v, d, 64));
  return v;
}

// OP over groups of N consecutive lanes (N a power of two, groups aligned), the result in every lane of the group; the
// lanes of a group make the call together
template <int N, class OP, typename T>
__device__ __forceinline__ T group_reduce(T v) {
#pragma unroll
  for (int d = N / 2; d >= 1; d >>= 1) v = OP::of(v, __shfl_xor(v, d, 64));
  return v;
}

// Inclusive sum over the 64 lanes in lane order, by doubling: six steps, step d adding the partial sum that ends d
// lanes below.  The association is fixed, so a float scan gives the same bits in every run.
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// The two workgroup forms, for a one-dimensional workgroup of WAVES waves and WAVES words of LDS at `wave_tot`.
// Both publish one word per wave, barrier, read all the words, barrier.  The contract:
//   - every thread of the workgroup makes the call, in uniform control flow (it holds two __syncthreads());
//   - nobody reads wave_tot after the last barrier in front of the call: the call overwrites it without waiting;
//   - the first barrier puts every LDS write made before the call in front of every LDS access made after it, and
//     every LDS read made before the call in front of every LDS write made after it, so a caller may initialise or
//     reuse other LDS words around the call without a barrier of its own;
//   - the second barrier ends the reads of wave_tot: the scratch is free when the call returns, for the next call
//     or for anything else.

// Inclusive sum in thread order: the wave scan, then the totals of the waves in front added in wave order
// (((t0 + t1) + ...) + own scan).  `total`, the sum over the workgroup in the same order, goes to every thread.
template <int WAVES, typename T>
__device__ __forceinline__ T block_incl_scan(T v, T* wave_tot, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_incl_scan(v);
  if (lane == 63) wave_tot[wave] = v;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const T x = wave_tot[w];
    if (w < wave) base += x;
    tot += x;
  }
  __syncthreads();
  total = tot;
  return base + v;
}

// OP over the workgroup, the result in every thread
template <int WAVES, class OP, typename T>
__device__ __forceinline__ T block_reduce(T v, T* wave_tot) {
  v = wave_reduce<OP>(v);
  if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = wave_tot[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) r = OP::of(r, wave_tot[w]);
  __syncthreads();
  return r;
}

// ---- LDS-DMA and its hand-counted wait (gemm.hip, gemm_big.hip, mm_fp4.hip, prefill_fp8_kernel.h) ----
// global -> LDS without a register: every lane fetches 16 (or 4) bytes from its own `src`, the wave writes them
// linearly from `lds_dst` on (lane i -> byte 16 i resp. 4 i).  The builtin wants the size as a literal.
__device__ __forceinline__ void lds_dma16(const void* src, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}
__device__ __forceinline__ void lds_dma4(const void* src, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_dst, 4, 0, 0);
}

// Wait until at most VMCNT of this wave's memory instructions (the DMA pieces still allowed in flight) and none of
// its LDS accesses are outstanding, then the workgroup barrier -- `__syncthreads()` would drain vmcnt.  ONE asm
// statement: the s_barrier builtin is no memory fence for the compiler, which may hoist the next LDS reads between a
// separate wait and the barrier (seen in prefill_fp8_kernel.h).
template <int VMCNT>
__device__ __forceinline__ void wait_vmcnt_barrier() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(VMCNT) : "memory");
}

// ---- storage-type unpack: 16 bytes -> VEC floats ----
template <int DT>
struct KVTraits;

template <>
struct KVTraits<FI_DTYPE_BF16> {
  static constexpr int BYTES = 2, VEC = 8;
  static __device__ __forceinline__ void unpack(const u32x4& r, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = __builtin_bit_cast(float, r[i] << 16);
      f[2 * i + 1] = __builtin_bit_cast(float, r[i] & 0xffff0000u);
    }
  }
};
template <>
struct KVTraits<FI_DTYPE_F16> {
  static constexpr int BYTES = 2, VEC = 8;
  static __device__ __forceinline__ void unpack(const u32x4& r, float* f) {
    using h2 = __attribute__((ext_vector_type(2))) _Float16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t w = r[i];  // copy first: bit_cast of a vector-element lvalue reads element 0
      h2 h = __builtin_bit_cast(h2, w);
      f[2 * i] = (float)h[0];
      f[2 * i + 1] = (float)h[1];
    }
  }
};
template <>
struct KVTraits<FI_DTYPE_FP8_E4M3> {
  static constexpr int BYTES = 1, VEC = 16;
  static __device__ __forceinline__ void unpack(const u32x4& r, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[i], false);
      f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[i], true);
      f[4 * i] = lo[0];
      f[4 * i + 1] = lo[1];
      f[4 * i + 2] = hi[0];
      f[4 * i + 3] = hi[1];
    }
  }
};
template <>
struct KVTraits<FI_DTYPE_FP8_E5M2> {
  static constexpr int BYTES = 1, VEC = 16;
  static __device__ __forceinline__ void unpack(const u32x4& r, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x2 lo = __builtin_amdgcn_cvt_pk_f32_bf8((int)r[i], false);
      f32x2 hi = __builtin_amdgcn_cvt_pk_f32_bf8((int)r[i], true);
      f[4 * i] = lo[0];
      f[4 * i + 1] = lo[1];
      f[4 * i + 2] = hi[0];
      f[4 * i + 3] = hi[1];
    }
  }
};

// 16-bit float load / store with a runtime dtype (FI_DTYPE_F16 / FI_DTYPE_BF16).
__device__ __forceinline__ float load_f16_or_bf16(const void* p, int64_t idx, int dt) {
  if (dt == FI_DTYPE_BF16) {
    uint32_t u = ((const uint16_t*)p)[idx];
    return __builtin_bit_cast(float, u << 16);
  }
  return (float)((const _Float16*)p)[idx];
}
__device__ __forceinline__ uint16_t f32_to_bf16_bits(float x) {
  return __builtin_bit_cast(uint16_t, (__bf16)x);
}
__device__ __forceinline__ uint16_t f32_to_f16_bits(float x) {
  return __builtin_bit_cast(uint16_t, (_Float16)x);
}
__device__ __forceinline__ uint16_t f32_to_16bit(float x, int dt) {
  return dt == FI_DTYPE_BF16 ? f32_to_bf16_bits(x) : f32_to_f16_bits(x);
}

// VEC (8, 4 or 1) consecutive 16-bit values of a compile-time dtype <-> floats, as one access of VEC * 2 bytes; the
// address must be aligned to that size.  Stores round to nearest even.
template <int DT, int VEC>
__device__ __forceinline__ void load_16bit(const uint16_t* p, float* f) {
  if constexpr (VEC == 1) {
    f[0] = load_f16_or_bf16(p, 0, DT);
  } else {
    using words = __attribute__((ext_vector_type(VEC / 2))) uint32_t;
    const words r = *(const words*)p;
#pragma unroll
    for (int i = 0; i < VEC / 2; ++i) {
      const uint32_t w = r[i];
      if constexpr (DT == FI_DTYPE_BF16) {
        f[2 * i] = __builtin_bit_cast(float, w << 16);
        f[2 * i + 1] = __builtin_bit_cast(float, w & 0xffff0000u);
      } else {
        using h2 = __attribute__((ext_vector_type(2))) _Float16;
        const h2 h = __builtin_bit_cast(h2, w);
        f[2 * i] = (float)h[0];
        f[2 * i + 1] = (float)h[1];
      }
    }
  }
}
template <int DT, int VEC>
__device__ __forceinline__ void store_16bit(uint16_t* p, const float* f) {
  if constexpr (VEC == 1) {
    p[0] = f32_to_16bit(f[0], DT);
  } else {
    using words = __attribute__((ext_vector_type(VEC / 2))) uint32_t;
    words r;
#pragma unroll
    for (int i = 0; i < VEC / 2; ++i)
      r[i] = (uint32_t)f32_to_16bit(f[2 * i], DT) | ((uint32_t)f32_to_16bit(f[2 * i + 1], DT) << 16);
    *(words*)p = r;
  }
}
__device__ __forceinline__ float load_any_float(const void* p, int64_t idx, int dt) {
  if (dt == FI_DTYPE_F32) return ((const float*)p)[idx];
  return load_f16_or_bf16(p, idx, dt);
}
__device__ __forceinline__ void store_any_float(void* p, int64_t idx, float x, int dt) {
  if (dt == FI_DTYPE_F32)
    ((float*)p)[idx] = x;
  else
    ((uint16_t*)p)[idx] = f32_to_16bit(x, dt);
}

}  // namespace fi
#endif  // __HIPCC__
