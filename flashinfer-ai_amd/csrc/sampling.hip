// Sampling: softmax, categorical draws with top-k / top-p / min-p filters, renormalisation, speculative chains.
// ref: include/flashinfer/sampling.cuh, csrc/sampling.cu, csrc/renorm.cu, flashinfer/sampling.py.
//
// Shape.  One workgroup of 1024 threads (16 waves) per output row; a row is f32 [vocab] and is streamed from
// memory in 16-byte chunks (chunk c of thread t in step i is c = i * 1024 + t), so the cost of an operator is the
// number of passes it makes over the row.  Three building blocks:
//
//   radix_select   the exact threshold of a filter, without sorting: the row's values are mapped to 32-bit keys that
//                  order like the values, and the key of the pivot is fixed digit by digit (11 + 11 + 10 bits, one
//                  pass each) from a histogram in LDS.  The histogram holds 64-bit integers -- counts for top-k,
//                  probabilities in 2^-40 fixed point for top-p -- so its sums do not depend on the order of the
//                  atomic adds and every run gives the same bits.  The reference reaches its pivots by rejection
//                  rounds (sampling.cuh:835-945) or a ternary search (sampling.cuh:1592-1850), both data dependent.
//   sample_weighted  an inverse-CDF draw over w(x) >= 0 in one pass: every thread sums the weights of its own chunks,
//                  a fixed-order block scan of the 1024 sums finds the thread the uniform number falls into, and
//                  that thread's wave reads its chunks again (1/1024 of the row, one chunk per lane), scans the
//                  chunk sums and picks the entry.  Entries of weight 0 are never returned; when rounding leaves
//                  the target unreached the last positive entry is.
//   block_incl_scan  (common.h) a wave scan in lane order, then the 16 wave totals summed in index order.
//
// Streaming loops issue four 16-byte loads per thread ahead of their use (for_chunks) and the kernels are held to 64
// registers, so two workgroups stay resident per CU.  The select-based kernels pay for that cap with a few registers
// spilled to scratch (2-11 per lane, most in top_k_mask_logits); measured against the uncapped build, which keeps one
// workgroup per CU, the capped one is 3-19 % faster at batch 989 and within 6 % at batch 64.  Every loop is bounded by the row length, the batch or a
// constant; nothing waits on data.
#include <algorithm>

#include "common.h"

namespace fi {

constexpr int kSampThreads = 1024;
constexpr int kSampWaves = kSampThreads / 64;
constexpr int kRadixBins = 2048;
constexpr int kMaxGrid = 1 << 20;
constexpr int kMaxVocab = 1 << 22;  // with entries clamped to 2.0 a row's fixed-point mass stays below 2^63
constexpr float kFixedOne = 1099511627776.0f;  // 2^40: top-p masses are summed as integers of this unit

using u64 = unsigned long long;

struct SampSmem {
  u64 hist[kRadixBins];
  u64 utot[kSampWaves];
  u64 above;
  float ftot[kSampWaves];
  int sel_bin;
  int winner;
  int sampled;
  int last_valid;
};

// ---- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) ----
// key = seed, counter = (offset, output row, draw block): a draw depends on nothing else.
__device__ __forceinline__ void philox4x32_10(uint64_t seed, uint64_t offset, uint32_t row, uint32_t block,
                                              uint32_t out[4]) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t c0 = (uint32_t)offset, c1 = (uint32_t)(offset >> 32), c2 = row, c3 = block;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// j-th uniform number in [0, 1) of an output row (24 bits)
__device__ __forceinline__ float philox_uniform(uint64_t seed, uint64_t offset, uint32_t row, uint32_t j) {
  uint32_t r[4];
  philox4x32_10(seed, offset, row, j >> 2, r);
  return (float)(r[j & 3] >> 8) * 5.9604644775390625e-08f;
}

// ---- row access: chunk c = elements 4c .. 4c+3; entries past the row read as `fill` ----
struct Row {
  const float* p;
  int n;
  int nc;    // chunks
  bool vec;  // 16-byte loads are legal (n % 4 == 0 and an aligned base)
  __device__ Row(const float* base, int64_t row, int n_) : p(base + row * (int64_t)n_), n(n_), nc((n_ + 3) >> 2) {
    vec = (n_ & 3) == 0 && (((uintptr_t)p) & 15) == 0;
  }
  __device__ __forceinline__ f32x4 load(int c, float fill) const {
    if (vec) return *(const f32x4*)(p + 4 * c);
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = 4 * c + j < n ? p[4 * c + j] : fill;
    return r;
  }
};

__device__ __forceinline__ void store4(float* out, int n, bool vec, int c, f32x4 v) {
  if (vec) {
    *(f32x4*)(out + 4 * c) = v;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * c + j < n) out[4 * c + j] = v[j];
  }
}

// use(c, load(c)) for every chunk c of this thread, in ascending order, with kUnroll loads issued ahead of their use:
// two resident workgroups of single loads keep 32 KB per CU in flight, short of what the memory latency asks for.
constexpr int kUnroll = 4;
template <class LOAD, class USE>
__device__ __forceinline__ void for_chunks(int nc, LOAD load, USE use) {
  int c = threadIdx.x;
  for (; c + (kUnroll - 1) * kSampThreads < nc; c += kUnroll * kSampThreads) {
    f32x4 v[kUnroll];
#pragma unroll
    for (int i = 0; i < kUnroll; ++i) v[i] = load(c + i * kSampThreads);
#pragma unroll
    for (int i = 0; i < kUnroll; ++i) use(c + i * kSampThreads, v[i]);
  }
  for (; c < nc; c += kSampThreads) use(c, load(c));
}

// keys that order like the values; NaN and (for probabilities) everything <= 0 map to 0
__device__ __forceinline__ uint32_t prob_key(float x) { return x > 0.f ? __builtin_bit_cast(uint32_t, x) : 0u; }
__device__ __forceinline__ uint32_t logit_key(float x) {
  if (x != x) return 0u;
  const uint32_t b = __builtin_bit_cast(uint32_t, x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// Mass of an entry in units of 2^-40.  Top-p expects rows that sum to about 1; an entry is clamped to 2.0 (anything
// >= top_p crosses the target on its own), so even an unnormalised row of kMaxVocab entries cannot wrap the 64-bit
// sums.  Entries below 2^-40 carry no mass: they are never the pivot and add nothing to the mass above it.
__device__ __forceinline__ u64 prob_mass_fixed(float x) {
  return x > 0.f ? (u64)(fminf(x, 2.0f) * kFixedOne) : 0ull;
}

// The largest key T such that the weights of {key >= T} reach `target` (weights: KW(c, x, keys, wts) fills the four
// keys and integer weights of chunk c = x, weight 0 past the row).  0 when the whole row does not reach it.
// Three passes over the row.
template <class KW>
__device__ uint32_t radix_select(const Row& row, KW kw, u64 target, SampSmem& sm) {
  const int nc = row.nc;
  uint32_t prefix = 0, mask = 0;
  u64 above = 0;
#pragma unroll 1
  for (int lvl = 0; lvl < 3; ++lvl) {
    const int shift = lvl == 0 ? 21 : lvl == 1 ? 10 : 0;
    const int nb = lvl == 2 ? 1024 : 2048;
    for (int b = threadIdx.x; b < kRadixBins; b += kSampThreads) sm.hist[b] = 0;
    if (threadIdx.x == 0) sm.sel_bin = -1;
    __syncthreads();
    for_chunks(nc, [&](int c) { return row.load(c, 0.f); }, [&](int c, const f32x4& x) {
      uint32_t key[4];
      u64 wt[4];
      kw(c, x, key, wt);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((key[j] & mask) == prefix && wt[j] != 0) atomicAdd(&sm.hist[(key[j] >> shift) & (nb - 1)], wt[j]);
    });
    __syncthreads();
    // thread t owns bins nb-1-2t and nb-2-2t: a prefix scan over threads walks the bins downwards
    const int b0 = nb - 1 - 2 * (int)threadIdx.x, b1 = b0 - 1;
    const u64 h0 = b0 >= 0 ? sm.hist[b0] : 0, h1 = b1 >= 0 ? sm.hist[b1] : 0;
    u64 tot;
    const u64 inc = block_incl_scan<kSampWaves, u64>(h0 + h1, sm.utot, tot);
    const u64 exc = above + inc - h0 - h1;
    if (h0 != 0 && exc + h0 >= target) atomicMax(&sm.sel_bin, b0);
    if (h1 != 0 && exc + h0 + h1 >= target) atomicMax(&sm.sel_bin, b1);
    __syncthreads();
    const int sel = sm.sel_bin;
    if (sel < 0) return 0u;  // uniform: the row's weights stay below the target, keep everything
    if (sel == b0) sm.above = exc;
    if (sel == b1) sm.above = exc + h0;
    __syncthreads();
    above = sm.above;
    prefix |= (uint32_t)sel << shift;
    mask |= (uint32_t)(nb - 1) << shift;
  }
  return prefix;
}

template <bool LOGITS>
__device__ uint32_t select_top_k(const Row& row, int k, SampSmem& sm) {
  if (k <= 0 || k >= row.n) return 0u;
  return radix_select(
      row,
      [&](int c, const f32x4& x, uint32_t* key, u64* wt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          key[j] = LOGITS ? logit_key(x[j]) : prob_key(x[j]);
          wt[j] = 4 * c + j < row.n ? 1ull : 0ull;
        }
      },
      (u64)k, sm);
}

__device__ uint32_t select_top_p(const Row& row, float top_p, SampSmem& sm) {
  if (!(top_p < 1.f)) return 0u;
  const u64 target = top_p > 0.f ? (u64)(top_p * kFixedOne) : 0ull;
  return radix_select(
      row,
      [&](int c, const f32x4& x, uint32_t* key, u64* wt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          key[j] = prob_key(x[j]);
          wt[j] = prob_mass_fixed(x[j]);
        }
      },
      target, sm);
}

// One draw from weights W4(c) (>= 0, 0 past the row) with the uniform number u; see the file comment.
template <class W4>
__device__ int sample_weighted(W4 w4, int nc, float u, SampSmem& sm) {
  float m = 0.f;
  int last = -1;
  for_chunks(nc, w4, [&](int c, const f32x4& w) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (w[j] > 0.f) {
        m += w[j];
        last = 4 * c + j;
      }
  });
  if (threadIdx.x == 0) {
    sm.winner = kSampThreads;
    sm.sampled = -1;
    sm.last_valid = -1;
  }
  float total;  // the scan's first barrier orders the initialisation above (its contract, common.h)
  const float inc = block_incl_scan<kSampWaves, float>(m, sm.ftot, total);
  const float target = u * total;
  if (last >= 0) atomicMax(&sm.last_valid, last);
  if (inc > target) atomicMin(&sm.winner, (int)threadIdx.x);
  __syncthreads();
  // The thread the target falls into owns the chunks win, win + 1024, ...; its whole wave walks them, 64 at a
  // time (one chunk per lane), scans the chunk sums and lets the lane that crosses the target pick the entry.
  const int win = sm.winner;
  if (win < kSampThreads && (int)(threadIdx.x >> 6) == (win >> 6)) {
    const int lane = threadIdx.x & 63;
    float base = __shfl(inc - m, win & 63, 64);
    const int win_last = __shfl(last, win & 63, 64);
    bool found = false;
    for (int c0 = win; c0 < nc && !found; c0 += 64 * kSampThreads) {
      const int c = c0 + lane * kSampThreads;
      f32x4 w = {0.f, 0.f, 0.f, 0.f};
      if (c < nc) w = w4(c);
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (w[j] > 0.f) s += w[j];
      const float sinc = wave_incl_scan(s);
      const unsigned long long hit = __ballot(base + sinc > target);
      if (hit != 0) {
        found = true;
        if (lane == __ffsll(hit) - 1) {
          float cum = base + sinc - s;
          int pick = -1, lastpos = -1;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (w[j] > 0.f) {
              cum += w[j];
              lastpos = 4 * c + j;
              if (cum > target && pick < 0) pick = lastpos;
            }
          sm.sampled = pick >= 0 ? pick : lastpos >= 0 ? lastpos : win_last;
        }
      }
      base += __shfl(sinc, 63, 64);
    }
    if (!found && lane == 0) sm.sampled = win_last;  // rounding left the target unreached: the last positive entry
  }
  __syncthreads();
  int id = sm.sampled;
  if (id < 0) id = sm.last_valid;
  return id < 0 ? 0 : id;
}

enum SampleOp { OP_PROBS = 0, OP_LOGITS, OP_TOP_K, OP_TOP_P, OP_MIN_P, OP_TOP_K_TOP_P };

template <int OP>
__device__ void sample_row(const fi_sampling_params_t& P, int bx, SampSmem& sm) {
  int r = P.indices ? P.indices[bx] : bx;
  r = min(max(r, 0), P.num_rows - 1);
  const Row row(P.probs, r, P.vocab);
  const int pi = min(r, P.param_len - 1);  // per-request parameters belong to the row drawn from
  const float u = philox_uniform(P.philox_seed, P.philox_offset, (uint32_t)bx, 0);
  int id;
  if constexpr (OP == OP_LOGITS) {
    float mx = -INFINITY;
    for_chunks(row.nc, [&](int c) { return row.load(c, -INFINITY); }, [&](int c, f32x4 x) {
      mx = fmaxf(mx, fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));  // fmaxf drops NaN
    });
    mx = block_reduce<kSampWaves, RedMax>(mx, sm.ftot);
    id = sample_weighted(
        [&](int c) {
          f32x4 x = row.load(c, -INFINITY);
#pragma unroll
          for (int j = 0; j < 4; ++j) x[j] = fast_exp2((x[j] - mx) * kLog2e);
          return x;
        },
        row.nc, u, sm);
  } else if constexpr (OP == OP_MIN_P) {
    float mx = 0.f;
    for_chunks(row.nc, [&](int c) { return row.load(c, 0.f); }, [&](int c, f32x4 x) {
      mx = fmaxf(mx, fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
    });
    mx = block_reduce<kSampWaves, RedMax>(mx, sm.ftot);
    const float min_p = P.top_p_arr ? P.top_p_arr[pi] : P.top_p_val;
    const float thr = fminf(min_p, 1.f) * mx;  // min_p > 1 would keep nothing: the maximum always stays
    id = sample_weighted(
        [&](int c) {
          f32x4 x = row.load(c, 0.f);
#pragma unroll
          for (int j = 0; j < 4; ++j) x[j] = x[j] >= thr ? x[j] : 0.f;
          return x;
        },
        row.nc, u, sm);
  } else {
    uint32_t thr = 0;
    if constexpr (OP == OP_TOP_K || OP == OP_TOP_K_TOP_P)
      thr = select_top_k<false>(row, P.top_k_arr ? P.top_k_arr[pi] : P.top_k_val, sm);
    if constexpr (OP == OP_TOP_P || OP == OP_TOP_K_TOP_P)
      thr = max(thr, select_top_p(row, P.top_p_arr ? P.top_p_arr[pi] : P.top_p_val, sm));
    id = sample_weighted(
        [&](int c) {
          f32x4 x = row.load(c, 0.f);
#pragma unroll
          for (int j = 0; j < 4; ++j) x[j] = prob_key(x[j]) >= thr ? x[j] : 0.f;
          return x;
        },
        row.nc, u, sm);
  }
  if (threadIdx.x == 0) P.samples[bx] = id;
}

// A launch holds at most kMaxGrid workgroups (grid x block must stay below 2^32 threads); each walks the output
// rows bx, bx + grid, ...  The barrier keeps a row's last LDS reads ahead of the next row's first writes.
template <int OP>
__global__ void __launch_bounds__(kSampThreads, 8) sampling_kernel(fi_sampling_params_t P) {
  __shared__ SampSmem sm;
  for (int bx = blockIdx.x; bx < P.batch; bx += gridDim.x) {
    sample_row<OP>(P, bx, sm);
    __syncthreads();
  }
}

enum TransformOp { TR_SOFTMAX = 0, TR_TOP_P_RENORM, TR_TOP_K_RENORM, TR_TOP_K_MASK };

template <int OP>
__device__ void transform_row(const fi_row_transform_params_t& P, int bx, SampSmem& sm) {
  const Row row(P.in, bx, P.vocab);
  float* out = P.out + (int64_t)bx * P.vocab;
  const bool ovec = row.vec && (((uintptr_t)out) & 15) == 0;
  const int pi = min(bx, P.param_len - 1);
  if constexpr (OP == TR_SOFTMAX) {
    // pass 1: per-thread running (max, sum of 2^((x - max) * sc)); pass 2 reads again and writes.  The maximum is
    // subtracted before the scale is applied, so the exponent of an entry near the maximum carries no rounding of
    // x / temperature (at temperature 0.1 that rounding alone would cost 1e-5 of a probability near 1/2).
    const float t = P.scalar_arr ? P.scalar_arr[pi] : P.scalar_val;
    const float sc = kLog2e / t;
    float m = -INFINITY, s = 0.f;
    for_chunks(row.nc, [&](int c) { return row.load(c, -INFINITY); }, [&](int c, f32x4 x) {
      const float mn = fmaxf(m, fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
      if (mn > -INFINITY) {
        s = s * fast_exp2((m - mn) * sc) + fast_exp2((x[0] - mn) * sc) + fast_exp2((x[1] - mn) * sc) +
            fast_exp2((x[2] - mn) * sc) + fast_exp2((x[3] - mn) * sc);
        m = mn;
      }
    });
    const float mx = block_reduce<kSampWaves, RedMax>(m, sm.ftot);
    float total;
    block_incl_scan<kSampWaves, float>(m > -INFINITY ? s * fast_exp2((m - mx) * sc) : 0.f, sm.ftot, total);
    const float inv = 1.f / total;
    for_chunks(row.nc, [&](int c) { return row.load(c, -INFINITY); }, [&](int c, f32x4 x) {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = fast_exp2((x[j] - mx) * sc) * inv;
      store4(out, row.n, ovec, c, x);
    });
  } else if constexpr (OP == TR_TOP_K_MASK) {
    const uint32_t thr = select_top_k<true>(row, P.top_k_arr ? P.top_k_arr[pi] : P.top_k_val, sm);
    for_chunks(row.nc, [&](int c) { return row.load(c, -INFINITY); }, [&](int c, f32x4 x) {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = logit_key(x[j]) >= thr ? x[j] : -INFINITY;
      store4(out, row.n, ovec, c, x);
    });
  } else {
    uint32_t thr;
    if constexpr (OP == TR_TOP_K_RENORM)
      thr = select_top_k<false>(row, P.top_k_arr ? P.top_k_arr[pi] : P.top_k_val, sm);
    else
      thr = select_top_p(row, P.scalar_arr ? P.scalar_arr[pi] : P.scalar_val, sm);
    float s = 0.f;
    for_chunks(row.nc, [&](int c) { return row.load(c, 0.f); }, [&](int c, f32x4 x) {
#pragma unroll
      for (int j = 0; j < 4; ++j) s += (x[j] > 0.f && prob_key(x[j]) >= thr) ? x[j] : 0.f;
    });
    float total;
    block_incl_scan<kSampWaves, float>(s, sm.ftot, total);
    const float inv = 1.f / total;
    for_chunks(row.nc, [&](int c) { return row.load(c, 0.f); }, [&](int c, f32x4 x) {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = (x[j] > 0.f && prob_key(x[j]) >= thr) ? x[j] * inv : 0.f;
      store4(out, row.n, ovec, c, x);
    });
  }
}

template <int OP>
__global__ void __launch_bounds__(kSampThreads, 8) row_transform_kernel(fi_row_transform_params_t P) {
  __shared__ SampSmem sm;
  for (int bx = blockIdx.x; bx < P.batch; bx += gridDim.x) {
    transform_row<OP>(P, bx, sm);
    __syncthreads();
  }
}

__device__ void chain_row(const fi_chain_speculative_params_t& P, int bx, SampSmem& sm) {
  const int n = P.num_speculative_tokens, d = P.vocab;
  const int32_t* ids = P.draft_token_ids + (int64_t)bx * n;
  int32_t* out = P.output_token_ids + (int64_t)bx * (n + 1);
  uint32_t draw = 0;  // every thread walks the same stream of uniform numbers
  auto accepts = [&](int i) {
    const int id = min(max(ids[i], 0), d - 1);
    const float q = P.target_probs[((int64_t)bx * (n + 1) + i) * d + id];
    const float p = P.draft_probs[((int64_t)bx * n + i) * d + id];
    const float u = philox_uniform(P.philox_seed, P.philox_offset, (uint32_t)bx, draw++);
    return u * p < q;
  };
  int pos = n;
  for (int i = 0; i < n; ++i) {
    if (!accepts(i)) {
      pos = i;
      break;
    }
    if (threadIdx.x == 0) out[i] = min(max(ids[i], 0), d - 1);
  }
  int accepted = pos;
  for (int i = pos; i < n; ++i) accepted += accepts(i) ? 1 : 0;
  if (threadIdx.x == 0) {
    P.output_accepted_token_num[bx] += accepted;
    P.output_emitted_draft_token_num[bx] += pos;
  }
  // the first rejected position is drawn from relu(target - draft); the bonus position has no draft row
  const Row q(P.target_probs, (int64_t)bx * (n + 1) + pos, d);
  const Row p(P.draft_probs, pos < n ? (int64_t)bx * n + pos : 0, d);
  const bool has_p = pos < n;
  const float u = philox_uniform(P.philox_seed, P.philox_offset, (uint32_t)bx, draw++);
  const int id = sample_weighted(
      [&](int c) {
        f32x4 x = q.load(c, 0.f);
        if (has_p) {
          const f32x4 y = p.load(c, 0.f);
#pragma unroll
          for (int j = 0; j < 4; ++j) x[j] = fmaxf(x[j] - y[j], 0.f);
        }
        return x;
      },
      q.nc, u, sm);
  if (threadIdx.x == 0) {
    out[pos] = id;
    for (int i = pos + 1; i <= n; ++i) out[i] = -1;
  }
}

__global__ void __launch_bounds__(kSampThreads, 8) chain_speculative_kernel(fi_chain_speculative_params_t P) {
  __shared__ SampSmem sm;
  for (int bx = blockIdx.x; bx < P.batch; bx += gridDim.x) {
    chain_row(P, bx, sm);
    __syncthreads();
  }
}

static int check_sampling(const fi_sampling_params_t* p, const char* what) {
  FI_REQUIRE(p, "%s: null params", what);
  FI_REQUIRE(p->batch >= 0 && p->num_rows >= 0, "%s: negative batch", what);
  if (p->batch == 0) return 0;
  FI_REQUIRE(p->probs && p->samples, "%s: null tensor", what);
  FI_REQUIRE(p->vocab >= 1 && p->vocab <= kMaxVocab, "%s: vocab %d out of range [1, 2^22]", what, p->vocab);
  FI_REQUIRE(p->num_rows >= 1, "%s: no rows to draw from", what);
  FI_REQUIRE(p->indices || p->batch <= p->num_rows, "%s: batch %d exceeds the %d rows and no indices are given", what,
             p->batch, p->num_rows);
  FI_REQUIRE((!p->top_k_arr && !p->top_p_arr) || p->param_len >= 1, "%s: parameter array without a length", what);
  return 0;
}

template <int OP>
static int launch_sampling(const fi_sampling_params_t* p, const char* what, fi_stream_t stream) {
  if (int rc = check_sampling(p, what)) return rc;
  if (p->batch == 0) return 0;
  fi_sampling_params_t q = *p;
  if (q.param_len < 1) q.param_len = 1;
  sampling_kernel<OP><<<dim3(std::min(q.batch, kMaxGrid)), dim3(kSampThreads), 0, (hipStream_t)stream>>>(q);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}

template <int OP>
static int launch_transform(const fi_row_transform_params_t* p, const char* what, fi_stream_t stream) {
  FI_REQUIRE(p, "%s: null params", what);
  FI_REQUIRE(p->batch >= 0, "%s: negative batch", what);
  if (p->batch == 0) return 0;
  FI_REQUIRE(p->in && p->out, "%s: null tensor", what);
  FI_REQUIRE(p->vocab >= 1 && p->vocab <= kMaxVocab, "%s: vocab %d out of range [1, 2^22]", what, p->vocab);
  FI_REQUIRE((!p->top_k_arr && !p->scalar_arr) || p->param_len >= 1, "%s: parameter array without a length", what);
  fi_row_transform_params_t q = *p;
  if (q.param_len < 1) q.param_len = 1;
  row_transform_kernel<OP><<<dim3(std::min(q.batch, kMaxGrid)), dim3(kSampThreads), 0, (hipStream_t)stream>>>(q);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_sampling_from_probs(const fi_sampling_params_t* p, fi_stream_t s) {
  return launch_sampling<OP_PROBS>(p, "sampling_from_probs", s);
}
extern "C" FI_API int fi_sampling_from_logits(const fi_sampling_params_t* p, fi_stream_t s) {
  return launch_sampling<OP_LOGITS>(p, "sampling_from_logits", s);
}
extern "C" FI_API int fi_top_k_sampling_from_probs(const fi_sampling_params_t* p, fi_stream_t s) {
  return launch_sampling<OP_TOP_K>(p, "top_k_sampling_from_probs", s);
}
extern "C" FI_API int fi_top_p_sampling_from_probs(const fi_sampling_params_t* p, fi_stream_t s) {
  return launch_sampling<OP_TOP_P>(p, "top_p_sampling_from_probs", s);
}
extern "C" FI_API int fi_min_p_sampling_from_probs(const fi_sampling_params_t* p, fi_stream_t s) {
  return launch_sampling<OP_MIN_P>(p, "min_p_sampling_from_probs", s);
}
extern "C" FI_API int fi_top_k_top_p_sampling_from_probs(const fi_sampling_params_t* p, fi_stream_t s) {
  return launch_sampling<OP_TOP_K_TOP_P>(p, "top_k_top_p_sampling_from_probs", s);
}
extern "C" FI_API int fi_softmax(const fi_row_transform_params_t* p, fi_stream_t s) {
  return launch_transform<TR_SOFTMAX>(p, "softmax", s);
}
extern "C" FI_API int fi_top_p_renorm_probs(const fi_row_transform_params_t* p, fi_stream_t s) {
  return launch_transform<TR_TOP_P_RENORM>(p, "top_p_renorm_probs", s);
}
extern "C" FI_API int fi_top_k_renorm_probs(const fi_row_transform_params_t* p, fi_stream_t s) {
  return launch_transform<TR_TOP_K_RENORM>(p, "top_k_renorm_probs", s);
}
extern "C" FI_API int fi_top_k_mask_logits(const fi_row_transform_params_t* p, fi_stream_t s) {
  return launch_transform<TR_TOP_K_MASK>(p, "top_k_mask_logits", s);
}

extern "C" FI_API int fi_chain_speculative_sampling(const fi_chain_speculative_params_t* p, fi_stream_t stream) {
  FI_REQUIRE(p, "chain_speculative_sampling: null params");
  FI_REQUIRE(p->batch >= 0, "chain_speculative_sampling: negative batch");
  if (p->batch == 0) return 0;
  FI_REQUIRE(p->num_speculative_tokens >= 0, "chain_speculative_sampling: negative num_speculative_tokens");
  FI_REQUIRE(p->target_probs && p->output_token_ids && p->output_accepted_token_num &&
                 p->output_emitted_draft_token_num && (p->num_speculative_tokens == 0 || (p->draft_probs && p->draft_token_ids)),
             "chain_speculative_sampling: null tensor");
  FI_REQUIRE(p->vocab >= 1 && p->vocab <= kMaxVocab, "chain_speculative_sampling: vocab %d out of range [1, 2^22]",
             p->vocab);
  chain_speculative_kernel<<<dim3(std::min(p->batch, kMaxGrid)), dim3(kSampThreads), 0, (hipStream_t)stream>>>(*p);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}
