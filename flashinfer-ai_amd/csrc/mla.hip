// Multi-head Latent Attention (MLA) over a paged cache: planner, kernel and C-ABI entry points.
// ref semantics: BatchMLAPagedAttentionWrapper, flashinfer/mla.py:85-420 (absorbed form: one shared KV
// "head", Q.K^T over head_dim_ckv + head_dim_kpe = 576 dims, P.V over the first 512 = the ckv part).
//
// Work item = (request, tile of kMlaRows packed rows, kv chunk); packed row r of a request is
// (qo_idx = r / num_heads, head = r % num_heads).  One workgroup of 4 waves per item:
//   - the item's keys are staged 64 tokens at a time in LDS (576 x 16 bit per token, padded), the next tile
//     prefetched into registers while the current one is used;
//   - S = Q.K^T: wave w takes tokens 16w..16w+15 of the tile, 18 steps of mfma_f32_16x16x32 over K = 576,
//     Q held in registers for the whole walk;
//   - online softmax in base 2, row maxima and sums exchanged through LDS, P written to LDS as 16 bit;
//   - O += P.V: wave w owns output columns 128w..128w+127 (8 blocks of 16), V = the tile's first 512 columns.
// A request cut into several chunks writes f32 partial states to the float workspace; launch_merge_n merges
// them (ragged, one entry range per packed row).  Every plan value the kernel uses is read from the int
// workspace, so a captured run() stays correct after a re-plan.
// An e4m3 cache (and query) is upcast exactly to the 16-bit compute type on the way into LDS (into the Q fragments);
// from LDS onward there is one code.
#include <algorithm>
#include <vector>

#include "common.h"
#include "merge_kernel.h"
#include "mla_plan.h"

namespace fi {

constexpr int kMlaThreads = 256;
constexpr int kMlaLdsRow = kMlaQK + 8;            // 16-bit elements per staged token (16 B pad against conflicts)
// 16-byte chunks of a cached token whose elements take `esz` bytes: 72 (64 ckv + 8 kpe) at 16 bit, 36 (32 + 4) as e4m3
constexpr int mla_chunks_per_token(int esz) { return kMlaQK * esz / 16; }
// 16-byte loads per thread and 64-token tile: 18 at 16 bit, 9 as e4m3
constexpr int mla_loads_per_thread(int esz) { return kMlaTileKV * mla_chunks_per_token(esz) / kMlaThreads; }
static_assert(kMlaTileKV * mla_chunks_per_token(2) % kMlaThreads == 0 &&
                  kMlaTileKV * mla_chunks_per_token(1) % kMlaThreads == 0,
              "loads must tile the threads");

// the sizes a plan is cut for, the int workspace header and MlaItem: mla_plan.h

struct MlaParams {
  const void* q_nope;
  const void* q_pe;
  const void* ckv;
  const void* kpe;
  const int32_t* kv_indices;
  const int32_t* int_ws;  // plan: header, merge indptr, items
  float* part_v;          // [entries, 512] f32
  float* part_s;          // [entries] f32
  void* o;                // [nnz_qo, num_heads, 512] contiguous
  float* lse;             // optional [nnz_qo, num_heads]
  int64_t q_nope_stride_n, q_nope_stride_h, q_pe_stride_n, q_pe_stride_h;
  int64_t ckv_stride_page, ckv_stride_n, kpe_stride_page, kpe_stride_n;
  FastDiv page_div;
  int32_t page_size, num_heads, causal;
  float sm_scale_log2;  // sm_scale * log2(e)
  const float* sm_scale_log2_dev;  // optional (an e4m3 cache only): read in place of sm_scale_log2, once per workgroup
};

template <int DT>
struct MlaType;
template <>
struct MlaType<FI_DTYPE_F16> {
  using frag = __attribute__((ext_vector_type(8))) _Float16;
  static __device__ __forceinline__ f32x4 mfma(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint16_t from_f32(float x) { return f32_to_f16_bits(x); }
  // two f32 that f16 holds exactly (every e4m3 value is one), as one word; a NaN stays a NaN
  static __device__ __forceinline__ uint32_t pack_exact(float a, float b) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(a, b));
  }
};
template <>
struct MlaType<FI_DTYPE_BF16> {
  using frag = __attribute__((ext_vector_type(8))) __bf16;
  static __device__ __forceinline__ f32x4 mfma(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint16_t from_f32(float x) { return f32_to_bf16_bits(x); }
  // two f32 that bf16 holds exactly (every e4m3 value has 3 mantissa bits): the high halves; the quiet NaN the
  // fp8 convert gives (0x7fc00000) keeps its quiet bit
  static __device__ __forceinline__ uint32_t pack_exact(float a, float b) {
    return (__builtin_bit_cast(uint32_t, a) >> 16) | (__builtin_bit_cast(uint32_t, b) & 0xffff0000u);
  }
};

// 8 e4m3 bytes -> 8 elements of the compute type, exactly: all 254 finite codes are f16 and bf16 values (largest 448,
// smallest subnormal 2^-9), and the two NaN codes give NaN.  cvt_pk_f32_fp8 is the convert KVTraits<FP8_E4M3>::unpack uses.
template <int DT>
__device__ __forceinline__ void mla_upcast8(uint32_t lo, uint32_t hi, uint32_t* out) {
  const uint32_t w[2] = {lo, hi};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[h], false);
    const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[h], true);
    out[2 * h] = MlaType<DT>::pack_exact(a[0], a[1]);
    out[2 * h + 1] = MlaType<DT>::pack_exact(b[0], b[1]);
  }
}

struct MlaSmem {
  uint16_t kv[kMlaTileKV][kMlaLdsRow];
  uint16_t p[kMlaRows][kMlaTileKV + 8];
  float red_max[4][kMlaRows];
  float red_sum[4][kMlaRows];
};

// DT: the compute and output type.  KV8 / Q8: the cache / the query holds e4m3 bytes, upcast to DT on the way into LDS /
// into the Q fragments; from LDS onward all forms are one code.
template <int DT, bool KV8 = false, bool Q8 = false>
__global__ void __launch_bounds__(kMlaThreads) mla_paged_kernel(const MlaParams p) {
  using T = MlaType<DT>;
  using frag = typename T::frag;
  constexpr int kQB = Q8 ? 1 : 2, kKB = KV8 ? 1 : 2;  // bytes per stored element
  constexpr int kChunksPerToken = mla_chunks_per_token(kKB), kCkvChunks = kMlaCkv * kKB / 16;
  constexpr int kLoadsPerThread = mla_loads_per_thread(kKB);
  __shared__ MlaSmem sm;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int lrow = lane & 15;  // A-operand row / C column
  const int lgrp = lane >> 4;  // k group / C row group
  const int num_work = p.int_ws[kMlaHdrNumWork];
  const int32_t* merge_indptr = p.int_ws + kMlaHeaderBytes / 4;
  const MlaItem* items = (const MlaItem*)((const char*)p.int_ws + p.int_ws[kMlaHdrItemsOff]);
  const int H = p.num_heads;
  float sm_scale_log2 = p.sm_scale_log2;
  if constexpr (KV8) {
    if (p.sm_scale_log2_dev) sm_scale_log2 = *p.sm_scale_log2_dev;
  }

  for (int w = blockIdx.x; w < num_work; w += gridDim.x) {
    const MlaItem it = items[w];
    const int rows = it.qo_len * H;
    // ---- Q fragments: row lrow of the tile, k = 32 s + 8 lgrp .. +7 ----
    frag qf[kMlaQK / 32];
    {
      const int r = it.row0 + lrow;
      const bool ok = r < rows;
      const int qi = ok ? r / H : 0, h = ok ? r % H : 0;
      const int64_t tok = it.qo_start + qi;
      const char* qn = (const char*)p.q_nope + (tok * p.q_nope_stride_n + (int64_t)h * p.q_nope_stride_h) * kQB;
      const char* qp = (const char*)p.q_pe + (tok * p.q_pe_stride_n + (int64_t)h * p.q_pe_stride_h) * kQB;
#pragma unroll
      for (int s = 0; s < kMlaQK / 32; ++s) {
        const int k = 32 * s + 8 * lgrp;
        u32x4 v = {0, 0, 0, 0};
        if constexpr (Q8) {  // 8 bytes per fragment, upcast once, before the kv walk (zero bytes are zeros)
          u32x2 r = {0, 0};
          if (ok) r = k < kMlaCkv ? *(const u32x2*)(qn + k) : *(const u32x2*)(qp + (k - kMlaCkv));
          uint32_t u[4];
          mla_upcast8<DT>(r[0], r[1], u);
          v = u32x4{u[0], u[1], u[2], u[3]};
        } else {
          if (ok) v = k < kMlaCkv ? *(const u32x4*)(qn + k * 2) : *(const u32x4*)(qp + (k - kMlaCkv) * 2);
        }
        qf[s] = __builtin_bit_cast(frag, v);
      }
    }
    // causal: row of query qo_idx sees keys kv_idx <= kv_len - qo_len + qo_idx
    int kv_last[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = it.row0 + 4 * lgrp + i;
      kv_last[i] = p.causal ? it.kv_len - it.qo_len + (r < rows ? r / H : 0) : 0x7fffffff;
    }
    float m[4], l[4];
    f32x4 acc[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      m[i] = -1.0e30f;
      l[i] = 0.f;
    }
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- global -> registers for the tile starting at t0 (tokens past kv_end are zeros, never read) ----
    // (an e4m3 cache: the registers hold the raw bytes, 16 elements each, and half as many of them)
    u32x4 pre[kLoadsPerThread];
    auto load_tile = [&](int t0) {
#pragma unroll
      for (int i = 0; i < kLoadsPerThread; ++i) {
        const int c = tid + kMlaThreads * i;
        const int tk = c / kChunksPerToken, ch = c % kChunksPerToken;
        const int t = t0 + tk;
        u32x4 v = {0, 0, 0, 0};
        if (t < it.kv_end) {
          const int pi = (int)fast_div((uint32_t)t, p.page_div);
          const int entry = t - pi * p.page_size;
          const int64_t page = p.kv_indices[it.page_base + pi];
          if (ch < kCkvChunks)
            v = *(const u32x4*)((const char*)p.ckv + (page * p.ckv_stride_page + entry * p.ckv_stride_n) * kKB + ch * 16);
          else
            v = *(const u32x4*)((const char*)p.kpe + (page * p.kpe_stride_page + entry * p.kpe_stride_n) * kKB +
                                (ch - kCkvChunks) * 16);
        }
        pre[i] = v;
      }
    };
    load_tile(it.kv_start);
    for (int t0 = it.kv_start; t0 < it.kv_end; t0 += kMlaTileKV) {
      __syncthreads();  // the previous tile's LDS reads are done
#pragma unroll
      for (int i = 0; i < kLoadsPerThread; ++i) {
        const int c = tid + kMlaThreads * i;
        if constexpr (KV8) {
          // chunk ch holds elements 16 ch .. 16 ch + 15 of the token: the columns of the 16-bit chunks 2 ch, 2 ch + 1
          uint32_t u[8];
          mla_upcast8<DT>(pre[i][0], pre[i][1], u);
          mla_upcast8<DT>(pre[i][2], pre[i][3], u + 4);
          uint16_t* dst = &sm.kv[c / kChunksPerToken][(c % kChunksPerToken) * 16];
          *(u32x4*)dst = u32x4{u[0], u[1], u[2], u[3]};
          *(u32x4*)(dst + 8) = u32x4{u[4], u[5], u[6], u[7]};
        } else {
          *(u32x4*)&sm.kv[c / kChunksPerToken][(c % kChunksPerToken) * 8] = pre[i];
        }
      }
      __syncthreads();
      if (t0 + kMlaTileKV < it.kv_end) load_tile(t0 + kMlaTileKV);

      // ---- S = Q.K^T for tokens 16 wave .. +15 ----
      f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
      const uint16_t* krow = &sm.kv[16 * wave + lrow][8 * lgrp];
#pragma unroll
      for (int s = 0; s < kMlaQK / 32; ++s) {
        const frag kf = __builtin_bit_cast(frag, *(const u32x4*)(krow + 32 * s));
        s4 = T::mfma(qf[s], kf, s4);
      }
      // scale, mask, per-wave row maxima (C layout: row 4 lgrp + i, token 16 wave + lrow)
      const int t = t0 + 16 * wave + lrow;
      float sv[4], mx[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sv[i] = (t < it.kv_end && t <= kv_last[i]) ? s4[i] * sm_scale_log2 : -INFINITY;
        float x = sv[i];
        x = fmaxf(x, lane_xor<1>(x));
        x = fmaxf(x, lane_xor<2>(x));
        x = fmaxf(x, lane_xor<4>(x));
        x = fmaxf(x, lane_xor<8>(x));
        mx[i] = x;
      }
      if (lrow == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sm.red_max[wave][4 * lgrp + i] = mx[i];
      }
      __syncthreads();
      float alpha[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * lgrp + i;
        const float tm = fmaxf(fmaxf(sm.red_max[0][r], sm.red_max[1][r]), fmaxf(sm.red_max[2][r], sm.red_max[3][r]));
        const float mn = fmaxf(m[i], tm);
        alpha[i] = fast_exp2(m[i] - mn);
        m[i] = mn;
        const float pv = fast_exp2(sv[i] - mn);
        sm.p[r][16 * wave + lrow] = T::from_f32(pv);
        float x = pv;
        x += lane_xor<1>(x);
        x += lane_xor<2>(x);
        x += lane_xor<4>(x);
        x += lane_xor<8>(x);
        if (lrow == 0) sm.red_sum[wave][r] = x;
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * lgrp + i;
        l[i] = l[i] * alpha[i] + (sm.red_sum[0][r] + sm.red_sum[1][r]) + (sm.red_sum[2][r] + sm.red_sum[3][r]);
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[b][i] *= alpha[i];
      }
      // ---- O += P.V over this wave's 128 columns ----
#pragma unroll
      for (int ks = 0; ks < kMlaTileKV / 32; ++ks) {
        const frag pf = __builtin_bit_cast(frag, *(const u32x4*)&sm.p[lrow][32 * ks + 8 * lgrp]);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          const int col = 128 * wave + 16 * b + lrow;
          using s16x8 = __attribute__((ext_vector_type(8))) short;
          s16x8 vv;
#pragma unroll
          for (int j = 0; j < 8; ++j) vv[j] = (short)sm.kv[32 * ks + 8 * lgrp + j][col];
          acc[b] = T::mfma(pf, __builtin_bit_cast(frag, vv), acc[b]);
        }
      }
    }

    // ---- write: o / lse directly, or the f32 partial state of this chunk ----
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = it.row0 + 4 * lgrp + i;
      if (r >= rows) continue;
      const int64_t g = (int64_t)it.qo_start * H + r;  // packed global row == [token, head] of o / lse
      const bool empty = !(l[i] > 0.f);
      const float inv = empty ? 0.f : 1.0f / l[i];
      const float ls = empty ? FI_NEG_INF : m[i] + fast_log2(l[i]);
      if (it.chunk < 0) {
        uint16_t* o = (uint16_t*)p.o + g * kMlaCkv;
#pragma unroll
        for (int b = 0; b < 8; ++b) o[128 * wave + 16 * b + lrow] = T::from_f32(acc[b][i] * inv);
        if (p.lse && wave == 0 && lrow == 0) p.lse[g] = ls;
      } else {
        const int64_t e = (int64_t)merge_indptr[g] + it.chunk;
        float* v = p.part_v + e * kMlaCkv;
#pragma unroll
        for (int b = 0; b < 8; ++b) v[128 * wave + 16 * b + lrow] = acc[b][i] * inv;
        if (wave == 0 && lrow == 0) p.part_s[e] = ls;
      }
    }
    __syncthreads();  // LDS reuse by the next item
  }
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_batch_mla_plan(const fi_batch_mla_plan_params_t* a, int64_t* plan_info_out,
                                        fi_stream_t stream) {
  FI_REQUIRE(a && plan_info_out, "batch_mla_plan: null argument");
  FI_REQUIRE(a->pinned_int_ws && a->qo_indptr_h && a->kv_indptr_h && a->kv_len_arr_h,
             "batch_mla_plan: null argument");
  FI_REQUIRE(a->head_dim_ckv == kMlaCkv, "batch_mla_plan: unsupported head_dim_ckv %d (only 512)", a->head_dim_ckv);
  FI_REQUIRE(a->head_dim_kpe == kMlaKpe, "batch_mla_plan: unsupported head_dim_kpe %d (only 64)", a->head_dim_kpe);
  FI_REQUIRE(a->q_dtype == a->kv_dtype, "batch_mla_plan: q dtype %d and kv dtype %d differ (dtype mismatch)",
             a->q_dtype, a->kv_dtype);
  FI_REQUIRE(a->q_dtype == FI_DTYPE_F16 || a->q_dtype == FI_DTYPE_BF16,
             "batch_mla_plan: unsupported dtype %d (f16 / bf16)", a->q_dtype);
  FI_REQUIRE(a->batch_size >= 0 && a->page_size > 0 && a->num_heads > 0,
             "batch_mla_plan: bad batch size / page size / num_heads");
  FI_REQUIRE(a->qo_indptr_h[0] == 0, "batch_mla_plan: qo_indptr[0] must be 0");
  const int B = a->batch_size, H = a->num_heads;
  std::vector<int64_t> tiles(B), kvl(B);
  int64_t total_tiles = 0, max_kv = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t qo_len = a->qo_indptr_h[b + 1] - a->qo_indptr_h[b];
    FI_REQUIRE(qo_len >= 0, "batch_mla_plan: qo_indptr must be non-decreasing");
    kvl[b] = a->kv_len_arr_h[b];
    FI_REQUIRE(kvl[b] >= 0, "batch_mla_plan: negative kv length");
    const int64_t pages = a->kv_indptr_h[b + 1] - a->kv_indptr_h[b];
    FI_REQUIRE(pages * a->page_size >= kvl[b], "batch_mla_plan: request %d has %lld pages for %lld tokens", b,
               (long long)pages, (long long)kvl[b]);
    tiles[b] = ceil_div<int64_t>(qo_len * H, kMlaRows);
    total_tiles += tiles[b];
    max_kv = std::max(max_kv, kvl[b]);
  }
  const int64_t total_rows = (int64_t)a->qo_indptr_h[B] * H;
  FI_REQUIRE(total_rows < (1ll << 31), "batch_mla_plan: too many rows");

  // kv chunk: the smallest multiple of 64 tokens (>= 256) whose items fit one round of resident workgroups
  // (kMlaWgPerCu per CU); no split when the unsplit items already fill it.  Chunks grow until the partial states fit.
  const int64_t max_items = std::max<int64_t>(kMlaWgPerCu * (int64_t)fi_num_compute_units(), 1);
  auto items_at = [&](int64_t chunk) {
    int64_t n = 0;
    for (int b = 0; b < B; ++b) n += tiles[b] * std::max<int64_t>(ceil_div<int64_t>(kvl[b], chunk), 1);
    return n;
  };
  auto entries_at = [&](int64_t chunk) {
    int64_t n = 0;
    for (int b = 0; b < B; ++b) {
      const int64_t c = ceil_div<int64_t>(kvl[b], chunk);
      if (c > 1) n += (int64_t)(a->qo_indptr_h[b + 1] - a->qo_indptr_h[b]) * H * c;
    }
    return n;
  };
  const int64_t whole = std::max<int64_t>(ceil_div<int64_t>(max_kv, kMlaTileKV) * kMlaTileKV, kMlaTileKV);
  int64_t chunk = whole;
  if (a->fixed_split_size > 0) {
    chunk = std::min(whole, ceil_div<int64_t>(a->fixed_split_size, kMlaTileKV) * kMlaTileKV);
  } else if (total_tiles > 0 && total_tiles < max_items) {
    chunk = kMlaTileKV * smallest_fitting(kMlaMinChunk / kMlaTileKV, whole / kMlaTileKV,
                                          [&](int64_t n) { return items_at(n * kMlaTileKV) > max_items; });
    chunk = std::min(whole, chunk);
  }
  const int64_t max_entries = mla_max_entries(a->float_ws_bytes);
  while (chunk < whole && entries_at(chunk) > max_entries) chunk *= 2;
  chunk = std::min(chunk, whole);
  FI_REQUIRE(chunk < (1ll << 31), "batch_mla_plan: kv chunk too large");

  // int workspace: header | merge indptr [total_rows + 1] | items (per request and chunk, the row tiles that
  // read it are adjacent so that they run together and the later reads hit L2)
  const int64_t num_work = items_at(chunk);
  const int64_t items_off = mla_items_offset(total_rows);
  const int64_t used = items_off + num_work * (int64_t)sizeof(MlaItem);
  FI_REQUIRE((int64_t)a->int_ws_bytes >= used,
             "batch_mla_plan: int workspace too small (%zu bytes, need %lld)", a->int_ws_bytes, (long long)used);
  FI_REQUIRE(num_work < (1ll << 31), "batch_mla_plan: too many work items");
  char* ws = (char*)a->pinned_int_ws;
  int32_t* hdr = (int32_t*)ws;
  int32_t* mind = (int32_t*)(ws + kMlaHeaderBytes);
  MlaItem* items = (MlaItem*)(ws + items_off);
  bool split = false;
  int64_t e = 0, w = 0;
  for (int b = 0; b < B; ++b) {
    const int32_t qs = a->qo_indptr_h[b], qo_len = a->qo_indptr_h[b + 1] - qs;
    const int64_t nc = std::max<int64_t>(ceil_div<int64_t>(kvl[b], chunk), 1);
    for (int64_t r = 0; r < (int64_t)qo_len * H; ++r) {
      mind[(int64_t)qs * H + r] = (int32_t)e;
      if (nc > 1) e += nc;
    }
    split |= nc > 1;
    for (int64_t c = 0; c < nc; ++c)
      for (int64_t t = 0; t < tiles[b]; ++t) {
        MlaItem& it = items[w++];
        it.qo_start = qs;
        it.row0 = (int32_t)(t * kMlaRows);
        it.qo_len = qo_len;
        it.kv_start = (int32_t)(c * chunk);
        it.kv_end = (int32_t)std::min<int64_t>((c + 1) * chunk, kvl[b]);
        it.kv_len = (int32_t)kvl[b];
        it.page_base = a->kv_indptr_h[b];
        it.chunk = nc > 1 ? (int32_t)c : -1;
      }
  }
  mind[total_rows] = (int32_t)e;
  hdr[kMlaHdrMagic] = kMlaWsMagic;
  hdr[kMlaHdrNumWork] = (int32_t)num_work;
  hdr[kMlaHdrItemsOff] = (int32_t)items_off;
  hdr[kMlaHdrSplit] = split ? 1 : 0;

  // a graph plan launches a fixed grid (the kernel walks the work list in strides of the grid) and always
  // merges, so that the captured kernels do not depend on the page table
  const int64_t grid = a->enable_cuda_graph ? max_items : std::max<int64_t>(num_work, 1);
  for (int i = 0; i < FI_MLA_PLAN_INFO_LEN; ++i) plan_info_out[i] = 0;
  plan_info_out[FI_MLA_NUM_WORK] = num_work;
  plan_info_out[FI_MLA_GRID] = grid;
  plan_info_out[FI_MLA_TOTAL_ROWS] = total_rows;
  plan_info_out[FI_MLA_KV_CHUNK_SIZE] = chunk;
  plan_info_out[FI_MLA_SPLIT_KV] = split ? 1 : 0;
  plan_info_out[FI_MLA_ENABLE_CUDA_GRAPH] = a->enable_cuda_graph ? 1 : 0;
  plan_info_out[FI_MLA_NUM_HEADS] = H;
  plan_info_out[FI_MLA_BATCH_SIZE] = B;
  plan_info_out[FI_MLA_INT_BYTES_USED] = used;
  plan_info_out[FI_MLA_MERGE_INDPTR_OFFSET] = kMlaHeaderBytes;
  plan_info_out[FI_MLA_ITEMS_OFFSET] = items_off;
  plan_info_out[FI_MLA_NUM_ENTRIES] = e;
  plan_info_out[FI_MLA_V_OFFSET] = mla_v_offset(a->float_ws_bytes);
  plan_info_out[FI_MLA_PAGE_SIZE] = a->page_size;
  plan_info_out[FI_MLA_DTYPE] = a->q_dtype;
  plan_info_out[FI_MLA_MAGIC] = FI_MLA_PLAN_MAGIC;
  if (a->int_ws) FI_HIP_CALL(hipMemcpyAsync(a->int_ws, a->pinned_int_ws, used, hipMemcpyHostToDevice, (hipStream_t)stream));
  return 0;
}

extern "C" FI_API int fi_batch_mla_run(const int64_t* plan_info, int32_t plan_info_len,
                                       const fi_batch_mla_params_t* a, fi_stream_t stream) {
  FI_REQUIRE(plan_info && plan_info_len >= FI_MLA_PLAN_INFO_LEN && plan_info[FI_MLA_MAGIC] == FI_MLA_PLAN_MAGIC,
             "batch_mla_run: plan_info is not an MLA plan (call plan first)");
  FI_REQUIRE(a, "batch_mla_run: null params");
  FI_REQUIRE(a->q_nope && a->q_pe && a->ckv && a->kpe && a->kv_indices && a->o && a->int_ws && a->float_ws,
             "batch_mla_run: null tensor");
  FI_REQUIRE(a->dtype == plan_info[FI_MLA_DTYPE], "batch_mla_run: dtype %d differs from the plan's %lld", a->dtype,
             (long long)plan_info[FI_MLA_DTYPE]);
  FI_REQUIRE(a->num_heads == plan_info[FI_MLA_NUM_HEADS], "batch_mla_run: num_heads differs from the plan");
  FI_REQUIRE(a->page_size == plan_info[FI_MLA_PAGE_SIZE], "batch_mla_run: page_size differs from the plan");
  // the plan's merge indptr and work list cover exactly its rows; more q rows would go unwritten, fewer would be
  // read and written past the caller's tensors
  FI_REQUIRE((int64_t)a->num_rows == plan_info[FI_MLA_TOTAL_ROWS],
             "batch_mla_run: q has %d packed rows, the plan %lld", a->num_rows, (long long)plan_info[FI_MLA_TOTAL_ROWS]);
  FI_REQUIRE((int64_t)a->int_ws_bytes >= plan_info[FI_MLA_INT_BYTES_USED], "batch_mla_run: int workspace too small");
  const int64_t max_entries = mla_max_entries(a->float_ws_bytes);
  FI_REQUIRE(plan_info[FI_MLA_NUM_ENTRIES] <= max_entries && plan_info[FI_MLA_V_OFFSET] == mla_v_offset(a->float_ws_bytes),
             "batch_mla_run: float workspace differs from the plan's");
  // storage types: 0 = the tensors hold `dtype`; an e4m3 cache with either query, an e4m3 query with an e4m3 cache
  for (int32_t st : {a->q_fp8, a->kv_fp8}) {
    FI_REQUIRE(st != FI_DTYPE_FP8_E5M2, "batch_mla_run: an e5m2 query or cache is not supported (fp8 is e4m3)");
    FI_REQUIRE(st == 0 || st == FI_DTYPE_FP8_E4M3, "batch_mla_run: q_fp8 / kv_fp8 must be 0 or FI_DTYPE_FP8_E4M3, got %d", st);
  }
  const bool q8 = a->q_fp8 != 0, kv8 = a->kv_fp8 != 0;
  FI_REQUIRE(!(q8 && !kv8), "batch_mla_run: an fp8 query with a 16-bit cache is not supported (an fp8 query needs an "
                            "fp8 cache)");
  FI_REQUIRE(!q8 || a->dtype == FI_DTYPE_BF16, "batch_mla_run: an fp8 query computes and writes bf16 (dtype %d given)",
             a->dtype);
  FI_REQUIRE(!a->sm_scale_log2_dev || kv8, "batch_mla_run: sm_scale_log2_dev is read with an fp8 cache only");
  // 16-byte vector loads: last dims contiguous (checked by the caller), rows 16-byte aligned
  const int64_t q_strides[] = {a->q_nope_stride_n, a->q_nope_stride_h, a->q_pe_stride_n, a->q_pe_stride_h};
  const int64_t kv_strides[] = {a->ckv_stride_page, a->ckv_stride_n, a->kpe_stride_page, a->kpe_stride_n};
  for (int64_t s : q_strides)
    FI_REQUIRE(s % (q8 ? 16 : 8) == 0, q8 ? "batch_mla_run: strides of an fp8 query must be multiples of 16 elements"
                                          : "batch_mla_run: strides must be multiples of 8 elements");
  for (int64_t s : kv_strides)
    FI_REQUIRE(s % (kv8 ? 16 : 8) == 0, kv8 ? "batch_mla_run: strides of an fp8 cache must be multiples of 16 elements"
                                            : "batch_mla_run: strides must be multiples of 8 elements");
  FI_REQUIRE(((uintptr_t)a->q_nope | (uintptr_t)a->q_pe | (uintptr_t)a->ckv | (uintptr_t)a->kpe) % 16 == 0,
             "batch_mla_run: tensors must be 16-byte aligned");
  if (a->num_rows == 0) return 0;
  MlaParams p;
  p.q_nope = a->q_nope;
  p.q_pe = a->q_pe;
  p.ckv = a->ckv;
  p.kpe = a->kpe;
  p.kv_indices = a->kv_indices;
  p.int_ws = (const int32_t*)a->int_ws;
  p.part_s = (float*)a->float_ws;
  p.part_v = (float*)((char*)a->float_ws + plan_info[FI_MLA_V_OFFSET]);
  p.o = a->o;
  p.lse = a->lse;
  p.q_nope_stride_n = a->q_nope_stride_n;
  p.q_nope_stride_h = a->q_nope_stride_h;
  p.q_pe_stride_n = a->q_pe_stride_n;
  p.q_pe_stride_h = a->q_pe_stride_h;
  p.ckv_stride_page = a->ckv_stride_page;
  p.ckv_stride_n = a->ckv_stride_n;
  p.kpe_stride_page = a->kpe_stride_page;
  p.kpe_stride_n = a->kpe_stride_n;
  p.page_div = FastDiv((uint32_t)a->page_size);
  p.page_size = a->page_size;
  p.num_heads = a->num_heads;
  p.causal = a->causal ? 1 : 0;
  p.sm_scale_log2 = a->sm_scale * kLog2e;
  p.sm_scale_log2_dev = a->sm_scale_log2_dev;
  const int grid = (int)plan_info[FI_MLA_GRID];
  hipStream_t st = (hipStream_t)stream;
  if (q8)
    mla_paged_kernel<FI_DTYPE_BF16, true, true><<<dim3(grid), dim3(kMlaThreads), 0, st>>>(p);
  else if (kv8 && a->dtype == FI_DTYPE_BF16)
    mla_paged_kernel<FI_DTYPE_BF16, true><<<dim3(grid), dim3(kMlaThreads), 0, st>>>(p);
  else if (kv8)
    mla_paged_kernel<FI_DTYPE_F16, true><<<dim3(grid), dim3(kMlaThreads), 0, st>>>(p);
  else if (a->dtype == FI_DTYPE_BF16)
    mla_paged_kernel<FI_DTYPE_BF16><<<dim3(grid), dim3(kMlaThreads), 0, st>>>(p);
  else
    mla_paged_kernel<FI_DTYPE_F16><<<dim3(grid), dim3(kMlaThreads), 0, st>>>(p);
  FI_HIP_CALL(hipGetLastError());
  if (plan_info[FI_MLA_SPLIT_KV] || plan_info[FI_MLA_ENABLE_CUDA_GRAPH]) {
    // ragged merge over packed rows (num_heads = 1): rows of unsplit requests have no entries and are skipped
    MergeNParams mp{p.part_v, p.part_s, (const int32_t*)((const char*)a->int_ws + plan_info[FI_MLA_MERGE_INDPTR_OFFSET]),
                    a->o, a->lse, 0, (int32_t)plan_info[FI_MLA_TOTAL_ROWS], 1, kMlaCkv, FI_DTYPE_F32, a->dtype, 1};
    FI_HIP_CALL(launch_merge_n(mp, st));
  }
  return 0;
}
