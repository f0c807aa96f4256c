// The mixture-of-experts layer around the MXFP4-weight grouped GEMM (gemm_mxfp4.hip): routing, the permutation into
// the GEMM's row operand, the gated activation between the two GEMMs and the weighted sum of the expert outputs.
// ref: trtllm_fp4_block_scale_moe, flashinfer/fused_moe/core.py:1819-1948; contracts in include/fi_mi355.h.
// All of it is data movement and elementwise work: no MFMA here.
//
// route.     One wave per token.  Lane l holds logits l, l + 64, ... (up to 8, num_experts <= 512) in registers; each of
//            the top_k rounds takes the lane's best untaken entry and reduces (value, index) over the wave with the
//            order "larger value, then lower index", so ties resolve without another pass.  The sigmoid methods
//            (DeepSeekV3, Llama4) are a kernel of their own on the same layout and rounds: see moe_route_sigmoid_kernel.
// permute.   Four launches, no host round trip.  count: one wave per FI_MOE_SORT_BLOCK expanded indices builds the
//            histogram of its block over the local experts (LDS adds: a count does not depend on their order).  scan: one
//            workgroup turns the histograms into per-block offsets (a serial walk over the blocks per expert) and the
//            expert totals into m_indptr.  place: the same wave ranks its indices 64 at a time -- the lanes of one
//            expert are found by ballot, a lane's rank is the number of lower lanes with its expert -- on top of a
//            running count in LDS that only this wave writes, which makes the order inside an expert the order of the
//            expanded index.  gather: indexed by the rows of the scale tensor, padding included, as the quantiser is, so
//            that every scale byte is written; a row copies its token's e4m3 bytes and moves the scale bytes of each
//            128 k elements as one dword into the swizzled layout.
// gated act. The quantiser's shape (mxfp8_quantize.hip) with the activation in front: a thread owns 8 output columns,
//            the quad shares amax; the rule itself is mx_quant.h.
// finalize.  A thread owns 8 columns of a token and walks its slots in order.
// gather, gated act. and finalize give a row to a row team (common.h).  A scale row finds its group and operand row by
// mx_row_of_scale_row (mx_layout.h) on m_indptr, which every workgroup first copies to LDS.
//
// The fp8 block-scale layer (trtllm_fp8_block_scale_moe, core.py:1742-1816) around fi_group_gemm_fp8_nt_groupwise shares
// route, the three sorting launches of permute and finalize.  Its gather and its gated activation are kernels of their
// own further down: the scales are one f32 per 128 columns in a plain row-major tensor indexed by the permuted row, so a
// row needs no scale-row lookup and no m_indptr in LDS, only m_indptr[G] to tell whether it is live.
#include <math.h>

#include "common.h"
#include "fp8_block_quant.h"
#include "mx_layout.h"
#include "mx_quant.h"

namespace fi {

constexpr int kMoeThreads = 256;
constexpr int kMoeSlots = FI_MOE_MAX_EXPERTS / 64;  // logits per lane

// ---- route ----------------------------------------------------------------------------------------------------------
struct MoeRouteArgs {
  const void* logits;
  int32_t* ids;
  uint16_t* weights;
  int32_t num_tokens, num_experts, top_k, method;
};

// (value, index) of the better of two candidates: the larger value, then the lower index
__device__ __forceinline__ void moe_better(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// the better of every lane's (value, index), afterwards in every lane
__device__ __forceinline__ void moe_wave_best(float& v, int& i) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const int oi = __shfl_xor(i, off, 64);
    moe_better(v, i, ov, oi);
  }
}

// one top-k round: the wave's best entry whose slot bit in `taken` is clear; the lane that holds it sets the bit
__device__ __forceinline__ void moe_take_best(const float (&v)[kMoeSlots], uint32_t& taken, int lane, float& bv, int& bi) {
  bv = -INFINITY;
  bi = 0x7fffffff;  // no candidate: loses against every expert, also one at -inf
#pragma unroll
  for (int s = 0; s < kMoeSlots; ++s)
    if (!(taken >> s & 1)) moe_better(bv, bi, v[s], lane + 64 * s);
  moe_wave_best(bv, bi);
  // the callers' limits leave an untaken expert: bi is one, and the same in every lane
  if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
}

template <int DT>
__global__ void __launch_bounds__(kMoeThreads) moe_route_kernel(const MoeRouteArgs A) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * (kMoeThreads / 64) + (threadIdx.x >> 6);
  if (t >= A.num_tokens) return;  // whole waves leave
  const int E = A.num_experts;
  float v[kMoeSlots];
  uint32_t taken = 0;  // bit s: slot s is chosen already, or past the last expert
#pragma unroll
  for (int s = 0; s < kMoeSlots; ++s) {
    const int e = lane + 64 * s;
    float x = -INFINITY;
    if (e < E) {
      x = load_any_float(A.logits, (int64_t)t * E + e, DT);
      if (!(x == x)) x = -INFINITY;
    } else {
      taken |= 1u << s;
    }
    v[s] = x;
  }
  float sel_v[FI_MOE_MAX_TOP_K];
  int sel_i[FI_MOE_MAX_TOP_K];
#pragma unroll
  for (int r = 0; r < FI_MOE_MAX_TOP_K; ++r) {
    sel_v[r] = -INFINITY;
    sel_i[r] = 0;
    if (r < A.top_k) {  // top_k <= num_experts
      float bv;
      int bi;
      moe_take_best(v, taken, lane, bv, bi);
      sel_v[r] = bv;
      sel_i[r] = bi;
    }
  }
  // weights, every lane the same arithmetic; sel_v[0] is the row's maximum
  const float m = sel_v[0];
  float w[FI_MOE_MAX_TOP_K];
  if (A.method == FI_MOE_ROUTING_TOPK) {
#pragma unroll
    for (int r = 0; r < FI_MOE_MAX_TOP_K; ++r) w[r] = sel_v[r];
  } else {
    float ex[FI_MOE_MAX_TOP_K], chosen = 0.f;
#pragma unroll
    for (int r = 0; r < FI_MOE_MAX_TOP_K; ++r) {
      ex[r] = r < A.top_k ? expf(sel_v[r] - m) : 0.f;
      chosen += ex[r];
    }
    if (A.method == FI_MOE_ROUTING_RENORMALIZE) {
#pragma unroll
      for (int r = 0; r < FI_MOE_MAX_TOP_K; ++r) w[r] = ex[r] / chosen;
    } else {
      float all = 0.f;
#pragma unroll
      for (int s = 0; s < kMoeSlots; ++s) all += lane + 64 * s < E ? expf(v[s] - m) : 0.f;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) all += __shfl_xor(all, off, 64);
      float p[FI_MOE_MAX_TOP_K], psum = 0.f;
#pragma unroll
      for (int r = 0; r < FI_MOE_MAX_TOP_K; ++r) {
        p[r] = ex[r] / all;
        psum += p[r];
      }
#pragma unroll
      for (int r = 0; r < FI_MOE_MAX_TOP_K; ++r) w[r] = A.method == FI_MOE_ROUTING_DEFAULT ? p[r] : p[r] / psum;
    }
  }
#pragma unroll
  for (int r = 0; r < FI_MOE_MAX_TOP_K; ++r) {
    if (r < A.top_k && lane == r) {
      A.ids[(int64_t)t * A.top_k + r] = sel_i[r];
      A.weights[(int64_t)t * A.top_k + r] = f32_to_bf16_bits(w[r]);
    }
  }
}

// ---- route, the sigmoid methods -------------------------------------------------------------------------------------
struct MoeRouteSigmoidArgs {
  const void* logits;
  const void* bias;
  int32_t* ids;
  uint16_t* weights;
  int32_t num_tokens, num_experts, top_k, method;
  int32_t n_group, topk_group, epg;  // n_group 0: no groups, every expert is a candidate
  int32_t bias_dt;
  float scale;
};

// (largest, second largest) of a set and another one's (o1, o2), merged
__device__ __forceinline__ void moe_top2_merge(float& b1, float& b2, float o1, float o2) {
  b2 = fmaxf(fminf(b1, o1), fmaxf(b2, o2));
  b1 = fmaxf(b1, o1);
}

// The layout and the top_k rounds of moe_route_kernel on the key b = sigmoid(logit) + bias (DeepSeekV3) or the logit
// itself (Llama4).  With groups three steps come first.  (1) Every group's score, the sum of its two largest keys, lands
// in lane g: when a group is epg = 2^k <= 64 consecutive lanes of one slot by a width-epg xor-shuffle of (best,
// second) pairs, otherwise through LDS, where lane g walks the keys of group g.  (2) topk_group rounds of the same
// (value, lower index) reduction over the lanes' scores build the bit mask of the kept groups, the same in every lane.
// (3) The experts of the other groups are marked taken, so no key, whatever its sign, lets one of them win a round.
template <int DT>
__global__ void __launch_bounds__(kMoeThreads) moe_route_sigmoid_kernel(const MoeRouteSigmoidArgs A) {
  __shared__ float lds_key[kMoeThreads / 64][FI_MOE_MAX_EXPERTS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int t = blockIdx.x * (kMoeThreads / 64) + wave;
  const bool live = t < A.num_tokens;  // a wave past the last token loads and stores nothing, but stays for the barrier
  const int E = A.num_experts;
  const bool deepseek = A.method == FI_MOE_ROUTING_DEEPSEEK_V3;
  float key[kMoeSlots], sig[kMoeSlots];
  uint32_t taken = 0;  // bit s: slot s is chosen already, in a dropped group, or past the last expert
#pragma unroll
  for (int s = 0; s < kMoeSlots; ++s) {
    const int e = lane + 64 * s;
    key[s] = -INFINITY;
    sig[s] = 0.f;
    if (e >= E) taken |= 1u << s;
    if (e < E && live) {
      float x = load_any_float(A.logits, (int64_t)t * E + e, DT);
      if (!(x == x)) x = -INFINITY;
      sig[s] = 1.0f / (1.0f + expf(-x));
      key[s] = x;
      if (deepseek) {
        key[s] = sig[s] + load_any_float(A.bias, e, A.bias_dt);
        if (!(key[s] == key[s])) key[s] = -INFINITY;
      }
    }
  }
  if (A.n_group > 1) {
    const int epg = A.epg, G = A.n_group;
    float score = -INFINITY;  // lane g < G: the score of group g
    if (epg <= 64 && (epg & (epg - 1)) == 0) {
#pragma unroll
      for (int s = 0; s < kMoeSlots; ++s) {
        if (64 * s < E) {  // the same in every lane
          float b1 = key[s], b2 = -INFINITY;
          for (int off = 1; off < epg; off <<= 1) {
            const float o1 = __shfl_xor(b1, off, 64);
            const float o2 = __shfl_xor(b2, off, 64);
            moe_top2_merge(b1, b2, o1, o2);
          }
          // group g begins at expert g * epg: lane (g * epg) & 63 of slot (g * epg) >> 6
          const float got = __shfl(b1 + b2, (lane * epg) & 63, 64);
          if (lane < G && (lane * epg) >> 6 == s) score = got;
        }
      }
    } else {
#pragma unroll
      for (int s = 0; s < kMoeSlots; ++s)
        if (lane + 64 * s < E) lds_key[wave][lane + 64 * s] = key[s];
      __syncthreads();
      if (lane < G) {
        float b1 = -INFINITY, b2 = -INFINITY;
        for (int i = 0; i < epg; ++i) moe_top2_merge(b1, b2, lds_key[wave][lane * epg + i], -INFINITY);
        score = b1 + b2;
      }
    }
    if (!(score == score)) score = -INFINITY;  // +inf and -inf keys in one group
    bool out = lane >= G;  // this lane's group is kept already, or there is none
    unsigned long long kept = 0;
    for (int r = 0; r < A.topk_group; ++r) {  // topk_group <= n_group: a group is left in every round
      float bv = out ? -INFINITY : score;
      int bi = out ? 0x7fffffff : lane;
      moe_wave_best(bv, bi);
      if (bi == lane) out = true;
      kept |= 1ull << (bi & 63);
    }
#pragma unroll
    for (int s = 0; s < kMoeSlots; ++s) {
      const int e = lane + 64 * s;
      if (e < E && !(kept >> (e / epg) & 1)) taken |= 1u << s;
    }
  }
  float sel_s[FI_MOE_MAX_TOP_K], chosen = 0.f;
  int sel_i[FI_MOE_MAX_TOP_K];
#pragma unroll
  for (int r = 0; r < FI_MOE_MAX_TOP_K; ++r) {
    sel_s[r] = 0.f;
    sel_i[r] = 0;
    if (r < A.top_k) {  // top_k <= the number of candidates
      float bv;
      moe_take_best(key, taken, lane, bv, sel_i[r]);
      float mine = 0.f;
#pragma unroll
      for (int s = 0; s < kMoeSlots; ++s)
        if (sel_i[r] >> 6 == s) mine = sig[s];
      sel_s[r] = __shfl(mine, sel_i[r] & 63, 64);  // selection is by the key, the weight comes from the plain sigmoid
      chosen += sel_s[r];
    }
  }
#pragma unroll
  for (int r = 0; r < FI_MOE_MAX_TOP_K; ++r) {
    if (live && r < A.top_k && lane == r) {
      const float w = deepseek ? sel_s[r] * A.scale / (chosen + 1e-20f) : sel_s[r];
      A.ids[(int64_t)t * A.top_k + r] = sel_i[r];
      A.weights[(int64_t)t * A.top_k + r] = f32_to_bf16_bits(w);
    }
  }
}

// ---- permute --------------------------------------------------------------------------------------------------------
struct MoePermuteArgs {
  const int32_t* ids;
  const uint8_t* x;
  const uint8_t* x_sf;
  int32_t* m_indptr;
  int32_t* map;
  uint8_t* x_out;
  uint8_t* sf_out;
  uint16_t* weights_out;
  int32_t* hist;  // [num_blocks, G]: counts, then offsets of the block inside every expert
  int32_t* p2e;   // [n] expanded index of a permuted row
  int32_t n, top_k, hidden, nkb;
  int32_t offset, G, packed;
  int32_t num_blocks;
  int32_t sf_rows;
  int32_t tpr_log2;
};

// local expert of an entry of topk_ids, -1 when it is not in the window
__device__ __forceinline__ int moe_local_expert(const MoePermuteArgs& A, int32_t id) {
  const int e = (A.packed ? (int)((uint32_t)id & 0xffffu) : id) - A.offset;
  return (e >= 0 && e < A.G) ? e : -1;
}

__global__ void __launch_bounds__(64) moe_count_kernel(const MoePermuteArgs A) {
  __shared__ int32_t cnt[FI_MOE_MAX_EXPERTS];
  const int lane = threadIdx.x;
  for (int e = lane; e < A.G; e += 64) cnt[e] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * FI_MOE_SORT_BLOCK;
  for (int step = 0; step < FI_MOE_SORT_BLOCK / 64; ++step) {
    const int64_t i = base + step * 64 + lane;
    const int le = i < A.n ? moe_local_expert(A, A.ids[i]) : -1;
    if (le >= 0) atomicAdd(&cnt[le], 1);
  }
  __syncthreads();
  for (int e = lane; e < A.G; e += 64) A.hist[(int64_t)blockIdx.x * A.G + e] = cnt[e];
}

__global__ void __launch_bounds__(FI_MOE_MAX_EXPERTS) moe_scan_kernel(const MoePermuteArgs A) {
  __shared__ int32_t wave_tot[FI_MOE_MAX_EXPERTS / 64];
  const int e = threadIdx.x;
  int total = 0;
  if (e < A.G) {
    for (int b = 0; b < A.num_blocks; ++b) {
      const int64_t at = (int64_t)b * A.G + e;
      const int c = A.hist[at];
      A.hist[at] = total;
      total += c;
    }
  }
  int rows;  // threads past G add 0
  const int incl = block_incl_scan<FI_MOE_MAX_EXPERTS / 64>(total, wave_tot, rows);
  if (e < A.G) A.m_indptr[e] = incl - total;
  if (e == 0) A.m_indptr[A.G] = rows;
}

__global__ void __launch_bounds__(64) moe_place_kernel(const MoePermuteArgs A) {
  __shared__ int32_t run[FI_MOE_MAX_EXPERTS];  // next permuted row of every expert, for this block
  const int lane = threadIdx.x;
  for (int e = lane; e < A.G; e += 64) run[e] = A.m_indptr[e] + A.hist[(int64_t)blockIdx.x * A.G + e];
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * FI_MOE_SORT_BLOCK;
  for (int step = 0; step < FI_MOE_SORT_BLOCK / 64; ++step) {
    const int64_t i = base + step * 64 + lane;
    const int32_t id = i < A.n ? A.ids[i] : -1;
    const int le = i < A.n ? moe_local_expert(A, id) : -1;
    int rank = 0, count = 0;
    unsigned long long todo = __ballot(le >= 0);
    while (todo) {  // one turn per expert present among the 64
      const int e0 = __shfl(le, __ffsll((unsigned long long)todo) - 1, 64);
      const unsigned long long same = __ballot(le == e0);
      if (le == e0) {
        rank = __popcll(same & ((1ull << lane) - 1));
        count = __popcll(same);
      }
      todo &= ~same;
    }
    const int first = le >= 0 ? run[le] : 0;
    __syncthreads();  // every lane has read before the last lane of an expert moves its count on
    if (le >= 0 && rank == count - 1) run[le] = first + count;
    __syncthreads();
    if (i < A.n) {
      const int p = le >= 0 ? first + rank : -1;
      A.map[i] = p;
      if (p >= 0 && p < A.n) A.p2e[p] = (int32_t)i;
      if (A.weights_out) A.weights_out[i] = (uint16_t)((uint32_t)id >> 16);
    }
  }
}

__device__ __forceinline__ void moe_load_indptr(int32_t* dst, const int32_t* m_indptr, int G) {
  for (int i = threadIdx.x; i <= G; i += kMoeThreads) dst[i] = m_indptr[i];
  __syncthreads();
}

__global__ void __launch_bounds__(kMoeThreads) moe_gather_kernel(const MoePermuteArgs A) {
  __shared__ int32_t indptr[FI_MOE_MAX_EXPERTS + 1];
  moe_load_indptr(indptr, A.m_indptr, A.G);
  const RowTeam team = row_team<kMoeThreads>(A.tpr_log2, A.sf_rows);
  if (team.past_end) return;
  int group;
  const int p = mx_row_of_scale_row(indptr, A.G, team.row, A.n, group);
  int token = -1;
  if (p >= 0) {
    const int i = A.p2e[p];
    if (i >= 0 && i < A.n) token = i / A.top_k;
  }
  const int chunks = A.hidden / 16;  // 16 bytes each; 8 chunks are 128 k elements, one dword of scales
  for (int c = team.lane; c < chunks; c += team.size) {
    if (token >= 0)
      *(u32x4*)(A.x_out + (int64_t)p * A.hidden + c * 16) = *(const u32x4*)(A.x + (int64_t)token * A.hidden + c * 16);
    if ((c & 7) == 0) {
      const int kb = c >> 1;  // a multiple of 4
      uint32_t w = 0;
      if (token >= 0) w = *(const uint32_t*)(A.x_sf + (int64_t)token * A.nkb + kb);
      *(uint32_t*)(A.sf_out + mx_sf_offset((int)team.row, kb, A.nkb)) = w;
    }
  }
}

// The gather of the fp8 block-scale layer: a row per permuted row, rows past the local count included.  A live row
// copies its token's e4m3 bytes; the lane that copies the first 16 bytes of a 128-column block also moves the block's
// f32 scale, read through both strides of the caller's tensor, into the row-major [n, nkb] operand of the GEMM.  A row at
// or past m_indptr[G] gets the scale 1.0f and no bytes.
struct MoeGatherFp8Args {
  const uint8_t* x;
  const float* x_scale;
  const int32_t* m_indptr;
  const int32_t* p2e;
  uint8_t* x_out;
  float* scale_out;
  int64_t stride_kb, stride_t;
  int32_t n, top_k, hidden, nkb, G, tpr_log2;
};

__global__ void __launch_bounds__(kMoeThreads) moe_gather_fp8_block_kernel(const MoeGatherFp8Args A) {
  const RowTeam team = row_team<kMoeThreads>(A.tpr_log2, A.n);
  if (team.past_end) return;
  const int64_t p = team.row;
  int token = -1;
  if (p < A.m_indptr[A.G]) {
    const int i = A.p2e[p];
    if (i >= 0 && i < A.n) token = i / A.top_k;
  }
  const int chunks = A.hidden / 16;  // 16 bytes each; 8 chunks are 128 k elements, one scale
  for (int c = team.lane; c < chunks; c += team.size) {
    if (token >= 0)
      *(u32x4*)(A.x_out + p * A.hidden + c * 16) = *(const u32x4*)(A.x + (int64_t)token * A.hidden + c * 16);
    if ((c & 7) == 0) {
      const int kb = c >> 3;
      A.scale_out[p * A.nkb + kb] = token >= 0 ? A.x_scale[kb * A.stride_kb + token * A.stride_t] : 1.0f;
    }
  }
}

// ---- gated activation -----------------------------------------------------------------------------------------------
struct MoeActArgs {
  const uint16_t* x;
  const int32_t* m_indptr;
  const float* bias;
  const float* alpha;
  const float* beta;
  const float* limit;
  uint8_t* q;
  uint8_t* sf;
  int32_t cum_m, inter, nkb, G, sf_rows, tpr_log2;
};

__global__ void __launch_bounds__(kMoeThreads) moe_gated_act_kernel(const MoeActArgs A) {
  __shared__ int32_t indptr[FI_MOE_MAX_EXPERTS + 1];
  moe_load_indptr(indptr, A.m_indptr, A.G);
  const RowTeam team = row_team<kMoeThreads>(A.tpr_log2, A.sf_rows);
  if (team.past_end) return;
  int g;
  const int src = mx_row_of_scale_row(indptr, A.G, team.row, A.cum_m, g);
  const float alpha = A.alpha ? A.alpha[g] : 1.f;
  const float beta = A.beta ? A.beta[g] : 0.f;
  const float limit = A.limit ? A.limit[g] : INFINITY;
  const int I = A.inter;
  const uint16_t* const xr = A.x + (int64_t)max(src, 0) * 2 * I;
  const float* const br = A.bias ? A.bias + (int64_t)g * 2 * I : nullptr;
  for (int cc = team.lane; cc < I / 8; cc += team.size) {  // I / 8 is a multiple of 16: the lanes of a quad stay together
    const int col = cc * 8;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    if (src >= 0) {
      float x1[8], x2[8];
      load_16bit<FI_DTYPE_BF16, 8>(xr + col, x1);
      load_16bit<FI_DTYPE_BF16, 8>(xr + I + col, x2);
      if (br) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x4 b1 = *(const f32x4*)(br + col + 4 * h);
          const f32x4 b2 = *(const f32x4*)(br + I + col + 4 * h);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            x1[4 * h + j] += b1[j];
            x2[4 * h + j] += b2[j];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float gt = fminf(x2[j], limit);
        const float l = fminf(fmaxf(x1[j], -limit), limit) + beta;
        v[j] = gt * (1.0f / (1.0f + expf(-alpha * gt))) * l;
      }
    }
    const int e = mx_e4m3_exponent(mx_quad_max(mx_amax8(v)));
    if (src >= 0) *(u32x2*)(A.q + (int64_t)src * I + col) = mx_e4m3_pack8(v, e);
    if ((cc & 3) == 0) A.sf[mx_sf_offset((int)team.row, cc >> 2, A.nkb)] = src >= 0 ? (uint8_t)(e + 127) : (uint8_t)0;
  }
}

// The gated activation of the fp8 block-scale layer: plain SwiGLU, then the block rule of fp8_block_quant.h.  A row per
// row of x; a thread owns 8 output columns and the 16 lanes of a 128-column block share amax.  The team is at least 16
// lanes and I / 8 a multiple of 16, so the lanes of a block take every turn of the loop together.
struct MoeActFp8Args {
  const uint16_t* x;
  const int32_t* m_indptr;
  uint8_t* q;
  float* scale;
  int32_t cum_m, inter, nkb, G, tpr_log2;
};

__global__ void __launch_bounds__(kMoeThreads) moe_gated_act_fp8_block_kernel(const MoeActFp8Args A) {
  const RowTeam team = row_team<kMoeThreads>(A.tpr_log2, A.cum_m);
  if (team.past_end) return;
  const int64_t row = team.row;
  const bool live = row < A.m_indptr[A.G];  // the same in every lane of the team
  const int I = A.inter;
  const uint16_t* const xr = A.x + row * 2 * I;
  for (int cc = team.lane; cc < I / 8; cc += team.size) {
    const int col = cc * 8;
    float s = 1.0f;
    if (live) {
      float x1[8], x2[8], v[8];
      load_16bit<FI_DTYPE_BF16, 8>(xr + col, x1);
      load_16bit<FI_DTYPE_BF16, 8>(xr + I + col, x2);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = x2[j] * (1.0f / (1.0f + expf(-x2[j]))) * x1[j];
      u32x2 q;
      s = fp8_block_quantize8(v, q);
      *(u32x2*)(A.q + row * I + col) = q;
    }
    if ((cc & (kFp8BlockLanes - 1)) == 0) A.scale[row * A.nkb + cc / kFp8BlockLanes] = s;
  }
}

// ---- finalize -------------------------------------------------------------------------------------------------------
struct MoeFinalizeArgs {
  const uint16_t* y;
  const uint16_t* weights;
  const int32_t* map;
  const float* bias;
  const int32_t* m_indptr;
  uint16_t* out;
  int32_t num_tokens, top_k, hidden, G, rows, tpr_log2;
};

__global__ void __launch_bounds__(kMoeThreads) moe_finalize_kernel(const MoeFinalizeArgs A) {
  __shared__ int32_t indptr[FI_MOE_MAX_EXPERTS + 1];
  if (A.bias) moe_load_indptr(indptr, A.m_indptr, A.G);
  const RowTeam team = row_team<kMoeThreads>(A.tpr_log2, A.num_tokens);
  if (team.past_end) return;
  const int64_t token = team.row;
  int rows[FI_MOE_MAX_TOP_K], groups[FI_MOE_MAX_TOP_K];
  float w[FI_MOE_MAX_TOP_K];
#pragma unroll
  for (int j = 0; j < FI_MOE_MAX_TOP_K; ++j) {
    rows[j] = -1;
    groups[j] = 0;
    w[j] = 0.f;
    if (j < A.top_k) {
      const int p = A.map[token * A.top_k + j];
      if (p >= 0 && p < A.rows) {
        rows[j] = p;
        w[j] = __builtin_bit_cast(float, (uint32_t)A.weights[token * A.top_k + j] << 16);
        if (A.bias) {
          int lo = 0, hi = A.G;  // the last group whose first row is <= p
          while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (indptr[mid] <= p) lo = mid; else hi = mid;
          }
          groups[j] = lo;
        }
      }
    }
  }
  for (int c = team.lane; c < A.hidden / 8; c += team.size) {
    const int col = c * 8;
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
    for (int j = 0; j < FI_MOE_MAX_TOP_K; ++j) {
      if (rows[j] >= 0) {
        float yv[8];
        load_16bit<FI_DTYPE_BF16, 8>(A.y + (int64_t)rows[j] * A.hidden + col, yv);
        if (A.bias) {
          const float* const b = A.bias + (int64_t)groups[j] * A.hidden + col;
          const f32x4 b0 = *(const f32x4*)b, b1 = *(const f32x4*)(b + 4);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            yv[i] += b0[i];
            yv[4 + i] += b1[i];
          }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(w[j], yv[i], acc[i]);
      }
    }
    store_16bit<FI_DTYPE_BF16, 8>(A.out + token * A.hidden + col, acc);
  }
}

static bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p % a) == 0; }

// the limits of both route entry points on num_experts and top_k
static int moe_route_check(const char* who, int num_experts, int top_k) {
  FI_REQUIRE(num_experts >= 1 && num_experts <= FI_MOE_MAX_EXPERTS, "%s: num_experts %d is not in [1, %d]", who, num_experts,
             FI_MOE_MAX_EXPERTS);
  FI_REQUIRE(top_k >= 1 && top_k <= FI_MOE_MAX_TOP_K && top_k <= num_experts,
             "%s: top_k %d is not in [1, min(%d, num_experts %d)]", who, top_k, FI_MOE_MAX_TOP_K, num_experts);
  return 0;
}

// the limits of both permute entry points
static int moe_permute_check(const char* who, int num_tokens, int top_k, int hidden, int offset, int G) {
  FI_REQUIRE(num_tokens >= 0 && top_k >= 0 && hidden >= 0 && G >= 0 && offset >= 0,
             "%s: negative size (num_tokens %d, top_k %d, hidden %d, local_expert_offset %d, local_num_experts %d)", who,
             num_tokens, top_k, hidden, offset, G);
  FI_REQUIRE(G >= 1 && G <= FI_MOE_MAX_EXPERTS, "%s: local_num_experts %d is not in [1, %d]", who, G, FI_MOE_MAX_EXPERTS);
  FI_REQUIRE(top_k >= 1 && top_k <= FI_MOE_MAX_TOP_K, "%s: top_k %d is not in [1, %d]", who, top_k, FI_MOE_MAX_TOP_K);
  FI_REQUIRE(hidden > 0 && hidden % 128 == 0, "%s: hidden %d must be a positive multiple of 128", who, hidden);
  return 0;
}

// What the sort of both permute entry points (count, scan, place) reads, after the check of its workspace: block
// histograms, then the inverse map a.p2e, which the entry point's gather reads.  The gather's own fields stay as they are.
static int moe_sort_args(const char* who, MoePermuteArgs& a, const int32_t* ids, int32_t* m_indptr, int32_t* map,
                         uint16_t* weights_out, int32_t* workspace, int64_t workspace_bytes, int64_t n, int top_k, int offset,
                         int64_t G, bool packed) {
  const int64_t num_blocks = ceil_div<int64_t>(n, FI_MOE_SORT_BLOCK);
  const int64_t ws_need = (num_blocks * G + n) * 4;
  FI_REQUIRE(workspace_bytes >= ws_need, "%s: workspace holds %lld bytes, %lld needed", who, (long long)workspace_bytes,
             (long long)ws_need);
  a.ids = ids;
  a.m_indptr = m_indptr;
  a.map = map;
  a.weights_out = packed ? weights_out : nullptr;
  a.hist = workspace;
  a.p2e = workspace + num_blocks * G;
  a.n = (int32_t)n;
  a.top_k = top_k;
  a.offset = offset;
  a.G = (int32_t)G;
  a.packed = packed;
  a.num_blocks = (int32_t)num_blocks;
  return 0;
}

static void moe_sort_launch(const MoePermuteArgs& a, hipStream_t st) {
  moe_count_kernel<<<dim3((uint32_t)a.num_blocks), dim3(64), 0, st>>>(a);
  moe_scan_kernel<<<dim3(1), dim3(FI_MOE_MAX_EXPERTS), 0, st>>>(a);
  moe_place_kernel<<<dim3((uint32_t)a.num_blocks), dim3(64), 0, st>>>(a);
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_moe_route(const fi_moe_route_params_t* p, fi_stream_t stream) {
  FI_REQUIRE(p, "moe_route: null params");
  FI_REQUIRE(p->num_tokens >= 0 && p->num_experts >= 0 && p->top_k >= 0,
             "moe_route: negative size (num_tokens %d, num_experts %d, top_k %d)", p->num_tokens, p->num_experts, p->top_k);
  if (const int rc = moe_route_check("moe_route", p->num_experts, p->top_k)) return rc;
  FI_REQUIRE(p->method == FI_MOE_ROUTING_DEFAULT || p->method == FI_MOE_ROUTING_RENORMALIZE ||
                 p->method == FI_MOE_ROUTING_RENORMALIZE_NAIVE || p->method == FI_MOE_ROUTING_TOPK,
             "moe_route: routing method %d is not provided", p->method);
  FI_REQUIRE(p->dtype == FI_DTYPE_F32 || p->dtype == FI_DTYPE_BF16, "moe_route: dtype %d is not f32 or bf16", p->dtype);
  if (p->num_tokens == 0) return 0;
  FI_REQUIRE(p->logits && p->topk_ids && p->topk_weights, "moe_route: null tensor");
  MoeRouteArgs a{p->logits, p->topk_ids, p->topk_weights, p->num_tokens, p->num_experts, p->top_k, p->method};
  const uint32_t grid = (uint32_t)ceil_div<int64_t>(p->num_tokens, kMoeThreads / 64);
  if (p->dtype == FI_DTYPE_F32)
    moe_route_kernel<FI_DTYPE_F32><<<dim3(grid), dim3(kMoeThreads), 0, (hipStream_t)stream>>>(a);
  else
    moe_route_kernel<FI_DTYPE_BF16><<<dim3(grid), dim3(kMoeThreads), 0, (hipStream_t)stream>>>(a);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}

extern "C" FI_API int fi_moe_route_sigmoid(const fi_moe_route_sigmoid_params_t* p, fi_stream_t stream) {
  FI_REQUIRE(p, "moe_route_sigmoid: null params");
  FI_REQUIRE(p->num_tokens >= 0 && p->num_experts >= 0 && p->top_k >= 0 && p->n_group >= 0 && p->topk_group >= 0,
             "moe_route_sigmoid: negative size (num_tokens %d, num_experts %d, top_k %d, n_group %d, topk_group %d)",
             p->num_tokens, p->num_experts, p->top_k, p->n_group, p->topk_group);
  const bool deepseek = p->method == FI_MOE_ROUTING_DEEPSEEK_V3;
  FI_REQUIRE(deepseek || p->method == FI_MOE_ROUTING_LLAMA4, "moe_route_sigmoid: routing method %d is not provided",
             p->method);
  if (const int rc = moe_route_check("moe_route_sigmoid", p->num_experts, p->top_k)) return rc;
  FI_REQUIRE(p->dtype == FI_DTYPE_F32 || p->dtype == FI_DTYPE_BF16, "moe_route_sigmoid: dtype %d is not f32 or bf16",
             p->dtype);
  const bool groups = deepseek && p->n_group > 1;
  int epg = 0;
  if (!deepseek) {
    FI_REQUIRE(p->top_k == 1, "moe_route_sigmoid: Llama4 routing takes top_k 1, not %d", p->top_k);
  } else {
    FI_REQUIRE(p->bias_dtype == FI_DTYPE_F32 || p->bias_dtype == FI_DTYPE_BF16,
               "moe_route_sigmoid: bias_dtype %d is not f32 or bf16", p->bias_dtype);
    if (groups) {
      FI_REQUIRE(p->n_group <= 64, "moe_route_sigmoid: n_group %d is not in [0, 64]", p->n_group);
      FI_REQUIRE(p->num_experts % p->n_group == 0, "moe_route_sigmoid: num_experts %d is not a multiple of n_group %d",
                 p->num_experts, p->n_group);
      epg = p->num_experts / p->n_group;
      FI_REQUIRE(epg >= 2, "moe_route_sigmoid: num_experts %d / n_group %d leaves %d expert per group, 2 needed",
                 p->num_experts, p->n_group, epg);
      FI_REQUIRE(p->topk_group >= 1 && p->topk_group <= p->n_group, "moe_route_sigmoid: topk_group %d is not in [1, n_group %d]",
                 p->topk_group, p->n_group);
      FI_REQUIRE(p->top_k <= p->topk_group * epg, "moe_route_sigmoid: top_k %d exceeds the %d experts of topk_group %d groups",
                 p->top_k, p->topk_group * epg, p->topk_group);
    }
  }
  if (p->num_tokens == 0) return 0;
  FI_REQUIRE(p->logits && p->topk_ids && p->topk_weights, "moe_route_sigmoid: null tensor");
  FI_REQUIRE(!deepseek || p->bias, "moe_route_sigmoid: null tensor (DeepSeekV3 routing reads bias)");
  MoeRouteSigmoidArgs a{};
  a.logits = p->logits;
  a.bias = p->bias;
  a.ids = p->topk_ids;
  a.weights = p->topk_weights;
  a.num_tokens = p->num_tokens;
  a.num_experts = p->num_experts;
  a.top_k = p->top_k;
  a.method = p->method;
  a.n_group = groups ? p->n_group : 0;
  a.topk_group = groups ? p->topk_group : 0;
  a.epg = epg;
  a.bias_dt = p->bias_dtype;
  a.scale = p->routed_scaling_factor;
  const uint32_t grid = (uint32_t)ceil_div<int64_t>(p->num_tokens, kMoeThreads / 64);
  if (p->dtype == FI_DTYPE_F32)
    moe_route_sigmoid_kernel<FI_DTYPE_F32><<<dim3(grid), dim3(kMoeThreads), 0, (hipStream_t)stream>>>(a);
  else
    moe_route_sigmoid_kernel<FI_DTYPE_BF16><<<dim3(grid), dim3(kMoeThreads), 0, (hipStream_t)stream>>>(a);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}

extern "C" FI_API int fi_moe_permute_mxfp8(const fi_moe_permute_params_t* p, fi_stream_t stream) {
  FI_REQUIRE(p, "moe_permute_mxfp8: null params");
  if (const int rc = moe_permute_check("moe_permute_mxfp8", p->num_tokens, p->top_k, p->hidden, p->local_expert_offset,
                                       p->local_num_experts))
    return rc;
  if (p->num_tokens == 0) return 0;
  const int64_t n = (int64_t)p->num_tokens * p->top_k;
  const int64_t G = p->local_num_experts;
  const int64_t sf_rows = mx_sf_rows_grouped(n, G);
  FI_REQUIRE(sf_rows < (1ll << 31), "moe_permute_mxfp8: too many rows");
  FI_REQUIRE(p->topk_ids && p->x && p->x_sf && p->m_indptr && p->expanded_to_permuted && p->x_permuted && p->sf_permuted &&
                 p->workspace, "moe_permute_mxfp8: null tensor");
  FI_REQUIRE(aligned(p->x, 16) && aligned(p->x_permuted, 16) && aligned(p->x_sf, 4) && aligned(p->sf_permuted, 4),
             "moe_permute_mxfp8: x and x_permuted must be 16-byte aligned, x_sf and sf_permuted 4-byte aligned");
  const int64_t nkb = p->hidden / kMxBlock;
  FI_REQUIRE(p->sf_bytes >= sf_rows * nkb, "moe_permute_mxfp8: sf_permuted holds %lld bytes, %lld needed",
             (long long)p->sf_bytes, (long long)(sf_rows * nkb));
  MoePermuteArgs a{};
  if (const int rc = moe_sort_args("moe_permute_mxfp8", a, p->topk_ids, p->m_indptr, p->expanded_to_permuted,
                                   p->unpacked_weights, p->workspace, p->workspace_bytes, n, p->top_k, p->local_expert_offset,
                                   G, p->packed != 0))
    return rc;
  a.x = (const uint8_t*)p->x;
  a.x_sf = (const uint8_t*)p->x_sf;
  a.x_out = (uint8_t*)p->x_permuted;
  a.sf_out = (uint8_t*)p->sf_permuted;
  a.hidden = p->hidden;
  a.nkb = (int32_t)nkb;
  a.sf_rows = (int32_t)sf_rows;
  a.tpr_log2 = row_team_log2(p->hidden / 16, kMoeThreads);
  hipStream_t st = (hipStream_t)stream;
  moe_sort_launch(a, st);
  const uint32_t grid = (uint32_t)ceil_div<int64_t>(sf_rows, kMoeThreads >> a.tpr_log2);
  moe_gather_kernel<<<dim3(grid), dim3(kMoeThreads), 0, st>>>(a);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}

extern "C" FI_API int fi_moe_gated_act_mxfp8(const fi_moe_gated_act_params_t* p, fi_stream_t stream) {
  FI_REQUIRE(p, "moe_gated_act_mxfp8: null params");
  FI_REQUIRE(p->cum_m >= 0 && p->intermediate >= 0 && p->num_groups >= 0,
             "moe_gated_act_mxfp8: negative size (cum_m %d, intermediate %d, num_groups %d)", p->cum_m, p->intermediate,
             p->num_groups);
  FI_REQUIRE(p->num_groups >= 1 && p->num_groups <= FI_MOE_MAX_EXPERTS, "moe_gated_act_mxfp8: num_groups %d is not in [1, %d]",
             p->num_groups, FI_MOE_MAX_EXPERTS);
  FI_REQUIRE(p->intermediate > 0 && p->intermediate % 128 == 0,
             "moe_gated_act_mxfp8: intermediate %d must be a positive multiple of 128", p->intermediate);
  if (p->cum_m == 0) return 0;
  const int64_t sf_rows = mx_sf_rows_grouped(p->cum_m, p->num_groups);
  FI_REQUIRE(sf_rows < (1ll << 31), "moe_gated_act_mxfp8: too many rows");
  FI_REQUIRE(p->x && p->m_indptr && p->q && p->sf, "moe_gated_act_mxfp8: null tensor");
  FI_REQUIRE(aligned(p->x, 16) && aligned(p->q, 8) && (!p->bias || aligned(p->bias, 16)),
             "moe_gated_act_mxfp8: x and bias must be 16-byte aligned, q 8-byte aligned");
  const int64_t nkb = p->intermediate / kMxBlock;
  FI_REQUIRE(p->sf_bytes >= sf_rows * nkb, "moe_gated_act_mxfp8: sf holds %lld bytes, %lld needed", (long long)p->sf_bytes,
             (long long)(sf_rows * nkb));
  MoeActArgs a{};
  a.x = (const uint16_t*)p->x;
  a.m_indptr = p->m_indptr;
  a.bias = p->bias;
  a.alpha = p->alpha;
  a.beta = p->beta;
  a.limit = p->limit;
  a.q = (uint8_t*)p->q;
  a.sf = (uint8_t*)p->sf;
  a.cum_m = p->cum_m;
  a.inter = p->intermediate;
  a.nkb = (int32_t)nkb;
  a.G = p->num_groups;
  a.sf_rows = (int32_t)sf_rows;
  a.tpr_log2 = row_team_log2(p->intermediate / 8, kMoeThreads);
  const uint32_t grid = (uint32_t)ceil_div<int64_t>(sf_rows, kMoeThreads >> a.tpr_log2);
  moe_gated_act_kernel<<<dim3(grid), dim3(kMoeThreads), 0, (hipStream_t)stream>>>(a);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}

extern "C" FI_API int fi_moe_permute_fp8_block(const fi_moe_permute_fp8_block_params_t* p, fi_stream_t stream) {
  FI_REQUIRE(p, "moe_permute_fp8_block: null params");
  if (const int rc = moe_permute_check("moe_permute_fp8_block", p->num_tokens, p->top_k, p->hidden, p->local_expert_offset,
                                       p->local_num_experts))
    return rc;
  FI_REQUIRE(p->scale_stride_kb >= 0 && p->scale_stride_t >= 0,
             "moe_permute_fp8_block: negative stride of x_scale (%lld, %lld)", (long long)p->scale_stride_kb,
             (long long)p->scale_stride_t);
  if (p->num_tokens == 0) return 0;
  const int64_t n = (int64_t)p->num_tokens * p->top_k;
  const int64_t G = p->local_num_experts;
  FI_REQUIRE(n < (1ll << 31), "moe_permute_fp8_block: too many rows");
  FI_REQUIRE(p->topk_ids && p->x && p->x_scale && p->m_indptr && p->expanded_to_permuted && p->x_permuted &&
                 p->scale_permuted && p->workspace, "moe_permute_fp8_block: null tensor");
  FI_REQUIRE(aligned(p->x, 16) && aligned(p->x_permuted, 16) && aligned(p->x_scale, 4) && aligned(p->scale_permuted, 4),
             "moe_permute_fp8_block: x and x_permuted must be 16-byte aligned, x_scale and scale_permuted 4-byte aligned");
  MoePermuteArgs a{};
  if (const int rc = moe_sort_args("moe_permute_fp8_block", a, p->topk_ids, p->m_indptr, p->expanded_to_permuted,
                                   p->unpacked_weights, p->workspace, p->workspace_bytes, n, p->top_k, p->local_expert_offset,
                                   G, p->packed != 0))
    return rc;
  MoeGatherFp8Args g{};
  g.x = (const uint8_t*)p->x;
  g.x_scale = p->x_scale;
  g.m_indptr = p->m_indptr;
  g.p2e = a.p2e;
  g.x_out = (uint8_t*)p->x_permuted;
  g.scale_out = p->scale_permuted;
  g.stride_kb = p->scale_stride_kb;
  g.stride_t = p->scale_stride_t;
  g.n = (int32_t)n;
  g.top_k = p->top_k;
  g.hidden = p->hidden;
  g.nkb = p->hidden / kFp8Block;
  g.G = (int32_t)G;
  g.tpr_log2 = row_team_log2(p->hidden / 16, kMoeThreads);
  hipStream_t st = (hipStream_t)stream;
  moe_sort_launch(a, st);
  const uint32_t grid = (uint32_t)ceil_div<int64_t>(n, kMoeThreads >> g.tpr_log2);
  moe_gather_fp8_block_kernel<<<dim3(grid), dim3(kMoeThreads), 0, st>>>(g);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}

extern "C" FI_API int fi_moe_gated_act_fp8_block(const fi_moe_gated_act_fp8_block_params_t* p, fi_stream_t stream) {
  FI_REQUIRE(p, "moe_gated_act_fp8_block: null params");
  FI_REQUIRE(p->cum_m >= 0 && p->intermediate >= 0 && p->num_groups >= 0,
             "moe_gated_act_fp8_block: negative size (cum_m %d, intermediate %d, num_groups %d)", p->cum_m, p->intermediate,
             p->num_groups);
  FI_REQUIRE(p->num_groups >= 1 && p->num_groups <= FI_MOE_MAX_EXPERTS,
             "moe_gated_act_fp8_block: num_groups %d is not in [1, %d]", p->num_groups, FI_MOE_MAX_EXPERTS);
  FI_REQUIRE(p->intermediate > 0 && p->intermediate % kFp8Block == 0,
             "moe_gated_act_fp8_block: intermediate %d must be a positive multiple of 128", p->intermediate);
  if (p->cum_m == 0) return 0;
  FI_REQUIRE(p->x && p->m_indptr && p->q && p->scale, "moe_gated_act_fp8_block: null tensor");
  FI_REQUIRE(aligned(p->x, 16) && aligned(p->q, 8) && aligned(p->scale, 4),
             "moe_gated_act_fp8_block: x must be 16-byte aligned, q 8-byte aligned, scale 4-byte aligned");
  MoeActFp8Args a{};
  a.x = (const uint16_t*)p->x;
  a.m_indptr = p->m_indptr;
  a.q = (uint8_t*)p->q;
  a.scale = p->scale;
  a.cum_m = p->cum_m;
  a.inter = p->intermediate;
  a.nkb = p->intermediate / kFp8Block;
  a.G = p->num_groups;
  a.tpr_log2 = row_team_log2(p->intermediate / 8, kMoeThreads);  // intermediate / 8 >= 16: a team holds whole blocks
  const uint32_t grid = (uint32_t)ceil_div<int64_t>(p->cum_m, kMoeThreads >> a.tpr_log2);
  moe_gated_act_fp8_block_kernel<<<dim3(grid), dim3(kMoeThreads), 0, (hipStream_t)stream>>>(a);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}

extern "C" FI_API int fi_moe_finalize(const fi_moe_finalize_params_t* p, fi_stream_t stream) {
  FI_REQUIRE(p, "moe_finalize: null params");
  FI_REQUIRE(p->num_tokens >= 0 && p->top_k >= 0 && p->hidden >= 0 && p->num_groups >= 0 && p->rows >= 0,
             "moe_finalize: negative size (num_tokens %d, top_k %d, hidden %d, num_groups %d, rows %d)", p->num_tokens,
             p->top_k, p->hidden, p->num_groups, p->rows);
  FI_REQUIRE(p->top_k >= 1 && p->top_k <= FI_MOE_MAX_TOP_K, "moe_finalize: top_k %d is not in [1, %d]", p->top_k,
             FI_MOE_MAX_TOP_K);
  FI_REQUIRE(p->hidden > 0 && p->hidden % 8 == 0, "moe_finalize: hidden %d must be a positive multiple of 8", p->hidden);
  FI_REQUIRE(!p->bias || (p->num_groups >= 1 && p->num_groups <= FI_MOE_MAX_EXPERTS),
             "moe_finalize: num_groups %d is not in [1, %d]", p->num_groups, FI_MOE_MAX_EXPERTS);
  if (p->num_tokens == 0) return 0;
  FI_REQUIRE(p->weights && p->expanded_to_permuted && p->out && (p->rows == 0 || p->y), "moe_finalize: null tensor");
  FI_REQUIRE(!p->bias || p->m_indptr, "moe_finalize: null tensor (m_indptr is needed with a bias)");
  FI_REQUIRE(aligned(p->y, 16) && aligned(p->out, 16) && aligned(p->bias, 16),
             "moe_finalize: y, out and bias must be 16-byte aligned");
  MoeFinalizeArgs a{};
  a.y = (const uint16_t*)p->y;
  a.weights = p->weights;
  a.map = p->expanded_to_permuted;
  a.bias = p->bias;
  a.m_indptr = p->m_indptr;
  a.out = (uint16_t*)p->out;
  a.num_tokens = p->num_tokens;
  a.top_k = p->top_k;
  a.hidden = p->hidden;
  a.G = p->num_groups;
  a.rows = p->rows;
  a.tpr_log2 = row_team_log2(p->hidden / 8, kMoeThreads);
  const uint32_t grid = (uint32_t)ceil_div<int64_t>(p->num_tokens, kMoeThreads >> a.tpr_log2);
  moe_finalize_kernel<<<dim3(grid), dim3(kMoeThreads), 0, (hipStream_t)stream>>>(a);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}
