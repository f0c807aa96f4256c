// Batch paged-KV decode with an fp8 (e4m3) QUERY over an fp8 (e4m3) cache: both products on the fp8 matrix
// instructions, the cache bytes fed to them as they lie in memory (no upcast anywhere on the K / V path).
//
// Ownership is that of decode_mfma16_kernel.h: one wave per (work, kv head) item of the planner's work list, the GQA
// group (<= 16 query heads) as the 16 columns of the MFMAs, f32 partial states for a split kv axis (merged by the
// merge_n launch), 32-token tiles, no workgroup barrier.  What is this kernel's own:
//
//   S^T[16 kv][16 heads] = K Q^T   D = 128: ONE v_mfma_scale_f32_16x16x128_f8f6f4 per 16 rows (unit E8M0 scales)
//                                  D =  64: two v_mfma_f32_16x16x32_fp8_fp8
//   O^T[16 d][16 heads] += V^T P^T v_mfma_f32_16x16x32_fp8_fp8, k = the tile's 32 kv rows
//
// K never touches LDS.  The contraction index of Q K^T may be permuted freely as long as K and Q use the same
// permutation, so a lane loads the bytes of its K row that make whole 64-byte runs with its three neighbours
// (g = lane >> 4, c = lane & 15):
//   A = K: lane (c, g) holds K[16 h + c][64 j + 16 g .. + 16], j < D / 64   (global_load_dwordx4, straight into the
//          operand registers: register 4 j + w of the lane is word w of that piece)
//   B = Q: lane (c, g) holds Q[head c] at the same bytes                    (D / 16 registers for the whole kernel)
//   C    : s[h][j] = S[kv 16 h + 4 g + j][head c]
// V is loaded by the same lanes at the same byte offsets (one page lookup per lane and 16-row half serves K and V),
// written row-major into a wave-private LDS tile of 32 rows x D bytes (4 KB per wave at D = 128, against the 16 KB of
// 16-bit K | V images of the 16-bit-query kernel) and comes back transposed through ds_read_b64_tr_b8:
//   B = P: byte 4 h + j of the lane = e4m3(448 p[h][j])     (k index 8 g + 4 h + j <-> kv row 16 h + 4 g + j)
//   A = V^T: lane (c, g) holds V[those 8 rows][16 db + c]   (one transposed read per 16-column block db: in a 16-lane
//          group lanes 2 b, 2 b + 1 address the 16 bytes of row b and lane c receives byte c of rows 0 .. 7)
//   C    : o[db][j] = O[head c][16 db + 4 g + j]
// LDS swizzle: 16-byte chunk ch of row r sits at chunk ch ^ key(r).  A ds_write_b128 quarter (16 lanes: 16 consecutive
// rows, one chunk) and a transposed read half (32 lanes: rows {0..7, 16..23} or {8..15, 24..31}, one chunk) must each
// fill 256 bytes of banks: at 128-byte rows the key is ((r >> 1) & 7) ^ (bit 4 of r << 2), at 64-byte rows
// ((r >> 2) & 3) ^ (bit 4 of r << 1).
//
// Softmax, the reference's fp8 rule (hopper/variants.cuh:64-102, attention_updater.cuh:167-256) with the EXACT running
// maximum: m includes the current tile before P is formed, P8 = e4m3(448 2^(x - m)) <= 448, the row sum is taken from
// the unrounded P, and the output carries 1 / 448.  (The prefill kernel's stale maximum with headroom is not used:
// decode has one row per head and an idle vector pipe.)  m starts at the finite -1e30: a fully masked tile leaves the
// state untouched, an empty range gives o = 0, lse = FI_NEG_INF.
#pragma once
#include "decode_mfma16_kernel.h"

namespace fi {

using i32x8d = __attribute__((ext_vector_type(8))) int;
using i32x2d = __attribute__((ext_vector_type(2))) int;

// OUT16: dtype of a final (unsplit) output row; partial states are f32 whatever it is
template <int OUT16, int D>
__global__ void __launch_bounds__(kDecodeThreads, 2) decode_fp8_kernel(const DecodeKernelParams p) {
  static_assert(D == 64 || D == 128, "head_dim 64 / 128");
  constexpr int kTile = 32;
  constexpr int ROWB = D;       // bytes per V row in LDS
  constexpr int NLD = D / 64;   // 16-byte pieces a lane holds of a K (and of a V) row
  constexpr int DBLK = D / 16;
  constexpr float kP8Max = 448.f;

  __shared__ __attribute__((aligned(16))) char smem[kDecodeWaves][kTile * ROWB];  // per wave: the V tile

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  int lb;  // XCD-contiguous logical block id (see decode_kernel.h)
  {
    const int b = blockIdx.x, total = gridDim.x;
    const int xcd = b & 7, slot = b >> 3;
    const int qn = total >> 3, rn = total & 7;
    lb = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + slot;
  }
  const int item = lb * kDecodeWaves + wave;
  if (item >= p.num_items) return;
  char* const vb = smem[wave];
  const int lc = lane & 15, lg = lane >> 4;

  // ---- item -> (work, kv head), kv range: as decode_mfma16_kernel.h ----
  const int kv_head = item % p.num_kv_heads;
  const int work = item / p.num_kv_heads;
  int req = 0, kv_tile = work;
  if (p.request_indices) {
    if (p.block_valid_mask && !p.block_valid_mask[work]) return;
    req = p.request_indices[work];
    kv_tile = p.kv_tile_indices[work];
  }
  int page_begin = 0, kv_len;
  if (p.indptr) {
    page_begin = p.indptr[req];
    const int np = p.indptr[req + 1] - page_begin;
    kv_len = np > 0 ? (np - 1) * p.page_size + p.last_page_len[req] : 0;
  } else {
    kv_len = p.single_kv_len;
  }
  int chunk_base = 0;
  if (p.plan_window_left >= 0 && p.indptr) {
    const int np = p.indptr[req + 1] - page_begin;
    chunk_base = np > 0 ? max((np - 1) * p.page_size - p.plan_window_left, 0) / p.page_size * p.page_size : 0;
  }
  const int win_start = p.window_left >= 0 ? max(0, kv_len - 1 - p.window_left) : 0;
  const int G = p.group_size;  // <= 16 (checked on the host)
  const int kv_chunk_size = p.kv_chunk_size_ptr ? *p.kv_chunk_size_ptr : p.kv_chunk_size;
  int chunk_start = chunk_base + (p.split_kv ? kv_tile * kv_chunk_size : 0);
  const int chunk_end = p.split_kv ? min(chunk_start + kv_chunk_size, kv_len) : kv_len;
  if (win_start > chunk_start) chunk_start += (win_start - chunk_start) / kTile * kTile;
  const int head0 = kv_head * G;

  // ---- Q: the B operand, in registers for the whole kernel (lanes past the group alias its last head) ----
  u32x4 qw[NLD];
  {
    const char* qrow = (const char*)p.q + (int64_t)req * p.q_stride_n + (int64_t)(head0 + min(lc, G - 1)) * p.q_stride_h;
#pragma unroll
    for (int j = 0; j < NLD; ++j) qw[j] = *(const u32x4*)(qrow + 64 * j + 16 * lg);
  }
  const float c_log2 = p.sm_scale * kLog2e;

  // ---- K / V loads: lane (c, g) reads bytes 64 j + 16 g .. + 16 of row 16 h + c of the tile ----
  const int64_t thread_off = (int64_t)kv_head * p.kv_stride_h + 16 * lg;
  const uint32_t stride_page32 = (uint32_t)p.kv_stride_page, stride_n32 = (uint32_t)p.kv_stride_n;
  // rows past the chunk's end are read as its last row (finite bytes of this request; their logits are masked)
  auto fetch_pages = [&](int tok0, int (&pg)[2], int (&en)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kvi = max(min(tok0 + 16 * h + lc, chunk_end - 1), 0);
      const int pi = (int)fast_div((uint32_t)kvi, p.page_div);
      en[h] = kvi - pi * p.page_size;
      pg[h] = p.indices[page_begin + pi];
    }
  };
  struct Stage {
    u32x4 k[2][NLD], v[2][NLD];
  };
  auto issue_loads = [&](const int (&pg)[2], const int (&en)[2], Stage& st) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t off = (int64_t)((uint64_t)(uint32_t)pg[h] * stride_page32 +
                                    (uint64_t)(uint32_t)en[h] * stride_n32) + thread_off;
#pragma unroll
      for (int j = 0; j < NLD; ++j)
        st.k[h][j] = __builtin_nontemporal_load((const u32x4*)((const char*)p.k + off + 64 * j));
#pragma unroll
      for (int j = 0; j < NLD; ++j)
        st.v[h][j] = __builtin_nontemporal_load((const u32x4*)((const char*)p.v + off + 64 * j));
    }
  };
  auto v_key = [](int row) -> int {
    return D == 128 ? (((row >> 1) & 7) ^ (((row >> 4) & 1) << 2)) : (((row >> 2) & 3) ^ (((row >> 4) & 1) << 1));
  };
  int v_wr[2];  // write address of piece j = 0 of row 16 h + c; piece 1 (D = 128) is chunk + 4: address ^ 64
#pragma unroll
  for (int h = 0; h < 2; ++h) v_wr[h] = (16 * h + lc) * ROWB + ((lg ^ v_key(16 * h + lc)) << 4);
  // transposed read: lane i of row group g addresses row b = i >> 1 of the 8 rows {4 g .. + 3, 16 + 4 g .. + 3},
  // bytes 8 (i & 1) .. + 8 of chunk db
  int v_rd;
  {
    const int b = lc >> 1;
    const int row = 16 * (b >> 2) + 4 * lg + (b & 3);
    v_rd = row * ROWB + (v_key(row) << 4) + 8 * (lc & 1);
  }

  f32x4 o_acc[DBLK];
#pragma unroll
  for (int db = 0; db < DBLK; ++db) o_acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -1.0e30f, l_run = 0.f;

  const int n_tok = chunk_end - chunk_start;
  if (n_tok > 0) {
    const int ntiles = (n_tok + kTile - 1) / kTile;
    int pg[2], en[2];
    Stage st;
    fetch_pages(chunk_start, pg, en);
    issue_loads(pg, en, st);
    fetch_pages(chunk_start + kTile, pg, en);
    for (int t = 0; t < ntiles; ++t) {
      const int tile0 = chunk_start + t * kTile;
      // V of tile t -> LDS, K of tile t -> the operand registers (waits for the tile's loads)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < NLD; ++j) *(u32x4*)(vb + (v_wr[h] ^ (64 * j))) = st.v[h][j];
      u32x4 kw[2][NLD];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < NLD; ++j) kw[h][j] = st.k[h][j];
      __builtin_amdgcn_wave_barrier();
      if (t + 1 < ntiles) {
        issue_loads(pg, en, st);  // tile t + 1 streams in while tile t is consumed
        fetch_pages(tile0 + 2 * kTile, pg, en);
      }
      // ---- S^T = K Q^T ----
      f32x4 s_acc[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        if constexpr (D == 128) {
          const i32x8d a = {(int)kw[h][0][0], (int)kw[h][0][1], (int)kw[h][0][2], (int)kw[h][0][3],
                            (int)kw[h][1][0], (int)kw[h][1][1], (int)kw[h][1][2], (int)kw[h][1][3]};
          const i32x8d b = {(int)qw[0][0], (int)qw[0][1], (int)qw[0][2], (int)qw[0][3],
                            (int)qw[NLD - 1][0], (int)qw[NLD - 1][1], (int)qw[NLD - 1][2], (int)qw[NLD - 1][3]};
          s_acc[h] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, zero, /*A e4m3*/ 0, /*B e4m3*/ 0, 0,
                                                                      0x7F7F7F7F, 0, 0x7F7F7F7F);
        } else {
          s_acc[h] = zero;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const long a = __builtin_bit_cast(long, u32x2{kw[h][0][2 * ks], kw[h][0][2 * ks + 1]});
            const long b = __builtin_bit_cast(long, u32x2{qw[0][2 * ks], qw[0][2 * ks + 1]});
            s_acc[h] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, s_acc[h], 0, 0, 0);
          }
        }
      }
      if (tile0 + kTile > chunk_end || tile0 < win_start) {
        // register j of half h is kv row 16 h + 4 g + j; visible rows are [win_start, chunk_end).  A tile with no
        // visible row gets mx = -inf below: m_run keeps its finite value, alpha = 1 and every p = 0.
        const int lo = win_start - tile0 - 4 * lg, hi = chunk_end - tile0 - 4 * lg;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int row = 16 * h + j;
            s_acc[h][j] = (row >= lo && row < hi) ? s_acc[h][j] : -INFINITY;
          }
      }
      // ---- online softmax (base 2), exact running maximum ----
      float mx = fmaxf(fmaxf(fmaxf(s_acc[0][0], s_acc[0][1]), fmaxf(s_acc[0][2], s_acc[0][3])),
                       fmaxf(fmaxf(s_acc[1][0], s_acc[1][1]), fmaxf(s_acc[1][2], s_acc[1][3])));
      mx = reduce_rows<true>(mx);
      const float m_new = fmaxf(m_run, mx * c_log2);
      const float alpha = fast_exp2(m_run - m_new);
      m_run = m_new;
      float psum = 0.f;
      uint32_t pw[2];  // P8: byte 4 h + j = e4m3(448 p[h][j])
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float pv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          pv[j] = fast_exp2(__builtin_fmaf(s_acc[h][j], c_log2, -m_new));
          psum += pv[j];
          pv[j] *= kP8Max;
        }
        int w = __builtin_amdgcn_cvt_pk_fp8_f32(pv[0], pv[1], 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(pv[2], pv[3], w, true);
        pw[h] = (uint32_t)w;
      }
      l_run = l_run * alpha + psum;
      if (__any(alpha != 1.0f)) {
#pragma unroll
        for (int db = 0; db < DBLK; ++db) o_acc[db] *= alpha;
      }
      // ---- O^T += V^T P^T ----
      const long pfrag = __builtin_bit_cast(long, u32x2{pw[0], pw[1]});
#pragma unroll
      for (int db = 0; db < DBLK; ++db) {
        const i32x2d vt = __builtin_amdgcn_ds_read_tr8_b64_v2i32(
            (__attribute__((address_space(3))) i32x2d*)(vb + (v_rd ^ (db << 4))));
        o_acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(__builtin_bit_cast(long, vt), pfrag, o_acc[db], 0, 0, 0);
      }
      __builtin_amdgcn_wave_barrier();
    }
  }

  // ---- finalize and write (partial state or final output); P8 carried 448 ----
  l_run = reduce_rows<false>(l_run);
  const bool empty = !(l_run > 0.f);
  const float inv = empty ? 0.f : 1.0f / (l_run * kP8Max);
  const float lse_v = empty ? FI_NEG_INF : m_run + fast_log2(l_run);
  if (lc < G) {
    const int qo_head = head0 + lc;
    const int64_t out_row = p.split_kv ? (int64_t)(p.o_indptr ? p.o_indptr[req] : 0) + kv_tile : req;
    const int64_t ob = (out_row * p.num_qo_heads + qo_head) * D;
#pragma unroll
    for (int db = 0; db < DBLK; ++db) {
      const int d0 = 16 * db + 4 * lg;
      if (p.split_kv) {
        *(f32x4*)(p.tmp_o + ob + d0) = o_acc[db] * inv;
      } else {
        const uint32_t w0 = pack2<OUT16>(o_acc[db][0] * inv, o_acc[db][1] * inv);
        const uint32_t w1 = pack2<OUT16>(o_acc[db][2] * inv, o_acc[db][3] * inv);
        *(u32x2*)((uint16_t*)p.o + ob + d0) = u32x2{w0, w1};
      }
    }
    if (lg == 0) {
      if (p.split_kv) p.tmp_lse[out_row * p.num_qo_heads + qo_head] = lse_v;
      else if (p.lse) p.lse[out_row * p.num_qo_heads + qo_head] = lse_v;
    }
  }
}

}  // namespace fi
